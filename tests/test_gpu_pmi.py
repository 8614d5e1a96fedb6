"""GPU checks of the co-occurrence and PMI step (csrc/cooc.hip, include/snx.h "Co-occurrence and PMI"): snx.cooc and the
mirror package src.pmi over it.

Counts are integers, so parity is equality: with tests/golden/g18_pmi (what the reference's src/pmi produced on a small
corpus) for every un-normalised setting, and with the plain-Python restatement (tests/pmi_reference.py) on id rows that
stand on the edges of the three kernel forms (64 tokens, the LDS tile, the workspace).  A normalised cell is compared with
the reference under |got - ref| <= (C + 1) 2^-24 ref, C the cell's count in the un-normalised twin: the reference makes C
fp32 additions of positive terms, each rounding once, we round once.  PMI is compared with g18's numpy float64 values:
equal where those are 0.0 or -inf, within 4 float64 ulp elsewhere (the logarithm is the only operation that can differ,
and both libraries document theirs near 1 ulp)."""
import os

import numpy as np
import pytest
import torch

from tests import pmi_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G18 = os.path.join(ROOT, "tests", "golden", "g18_pmi")
PMI_ULPS = 4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g18():
    return R.load_g18(G18)


def _fit(g18, s, dev, **kw):
    from src.pmi import CooccurrenceConfig, CooccurrenceMatrixBuilder, WindowType
    cfg = CooccurrenceConfig(WindowType(s["window_type"]), s["window_size"], s["min_term_freq"], s["max_vocab_size"],
                             s["symmetric"], s["normalize"])
    return CooccurrenceMatrixBuilder(cfg, device=dev, **kw).fit(g18["corpus"], show_progress=False)


def _golden(g18, name):
    a = g18["arrays"]
    return a[f"{name}/indptr"], a[f"{name}/indices"], a[f"{name}/data"]


def _text_side_equal(b, s):
    vocab = b.get_vocabulary()
    assert list(vocab) == s["vocab"] and sorted(vocab, key=vocab.get) == s["vocab"], s["name"]
    assert b.get_term_frequencies() == s["term_freq"] and b.get_document_frequencies() == s["doc_freq"], s["name"]
    assert b.get_stats().total_windows == s["total_windows"] and b.get_stats().total_cooccurrences == s["nnz"], s["name"]


# ------------------------------------------------------------------------------------------------ 1, 2: the goldens
def test_golden_counts_equal_the_reference(g18, dev):
    seen = 0
    for s in g18["settings"]:
        if s["normalize"]:
            continue
        b = _fit(g18, s, dev)
        _text_side_equal(b, s)
        data, indices, indptr = b.cooccurrence_csr()
        g_indptr, g_indices, g_data = _golden(g18, s["name"])
        assert data.dtype == np.float32 and indices.dtype == np.int32 and indptr.dtype == np.int64
        assert np.array_equal(indptr, g_indptr) and np.array_equal(indices, g_indices), s["name"]
        assert np.array_equal(data, g_data), s["name"]
        counts = b.cooccurrence_counts()
        assert counts.dtype == np.int64 and np.array_equal(counts, g_data.astype(np.int64)), s["name"]
        seen += 1
    assert seen == 11


def test_golden_normalized_within_the_derived_bound(g18, dev):
    seen = 0
    for s in g18["settings"]:
        if not s["normalize"]:
            continue
        b = _fit(g18, s, dev)
        _text_side_equal(b, s)
        data, indices, indptr = b.cooccurrence_csr()
        g_indptr, g_indices, g_data = _golden(g18, s["name"])
        c_indptr, c_indices, c_data = _golden(g18, s["name"].replace("_norm", "_count"))
        assert np.array_equal(indptr, g_indptr) and np.array_equal(indices, g_indices), s["name"]
        assert np.array_equal(c_indptr, g_indptr) and np.array_equal(c_indices, g_indices) and b.cooccurrence_counts() is None
        ref, C = g_data.astype(np.float64), c_data.astype(np.float64)
        gap = np.abs(data.astype(np.float64) - ref)
        print(f"{s['name']}: largest |got - ref| / ((C + 1) 2^-24 ref) = {(gap / ((C + 1) * 2.0 ** -24 * ref)).max():.3f}")
        assert (gap <= (C + 1) * 2.0 ** -24 * ref).all(), s["name"]
        again = _fit(g18, s, dev).cooccurrence_csr()                       # bit-identical from run to run
        assert again[0].tobytes() == data.tobytes() and np.array_equal(again[1], indices)
        seen += 1
    assert seen == 2


# ------------------------------------------------------------------------------------------------ 3: ids against the restatement
def _check_rows(rows, V, dev, symmetric, window_size=None, normalize=False, fast=False, **kw):
    from snx import cooc
    got = cooc.cooccurrence(*cooc.id_rows(rows), V, window_size=window_size, symmetric=symmetric, normalize=normalize,
                            device=dev, **kw)
    indptr, indices, data, counts, total = R.cooccurrence(rows, V, window_size, symmetric, normalize, fast=fast)
    assert got.shape == (V, V) and got.total_windows == total
    assert got.indptr.dtype == torch.long and got.indices.dtype == torch.int32 and got.data.dtype == torch.float32
    assert np.array_equal(got.indptr.cpu().numpy(), indptr) and np.array_equal(got.indices.cpu().numpy(), indices)
    assert got.data.cpu().numpy().tobytes() == data.tobytes()
    if normalize:
        assert got.counts is None
    else:
        assert got.counts.dtype == torch.long and np.array_equal(got.counts.cpu().numpy(), counts)
        assert counts.size == 0 or counts.max() < 2 ** 20                  # 2^24 is never approached
    return got


def _random_row(rng, n, V, oov=0.1):
    ids = rng.integers(0, V, size=n)
    ids[rng.random(n) < oov] = -1
    return ids.tolist()


@pytest.mark.parametrize("symmetric", [True, False])
def test_window_lengths_on_the_edges_of_the_forms(dev, symmetric):
    from snx import cooc
    assert cooc.LDS_TOKENS == 4096 and cooc.WAVE_TOKENS == 64
    rng = np.random.default_rng(18)
    T = cooc.LDS_TOKENS
    rows = [_random_row(rng, n, 40) for n in (0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1)]
    _check_rows(rows, 40, dev, symmetric, fast=True)
    _check_rows(rows[:5], 40, dev, symmetric)                              # one wave a window only
    _check_rows(rows[:9], 40, dev, symmetric, fast=True)                   # no workspace


@pytest.mark.parametrize("symmetric", [True, False])
def test_long_window_takes_the_workspace(dev, symmetric):
    rng = np.random.default_rng(19)
    _check_rows([_random_row(rng, 5000, 40, oov=0.05), [3, 4]], 40, dev, symmetric, fast=True)


@pytest.mark.parametrize("symmetric", [True, False])
def test_degenerate_windows_and_vocabularies(dev, symmetric):
    got = _check_rows([[7] * 9], 10, dev, symmetric)                       # one repeated term: the diagonal only
    assert got.indices.tolist() == [7] and got.counts.tolist() == [72 if symmetric else 36]
    assert _check_rows([[-1] * 5, [-1], []], 4, dev, symmetric).nnz == 0   # nothing in the vocabulary
    _check_rows([[-1, 2, -1, -1, 0, -1, 2, 3, -1], [-1, 1], [1, -1]], 4, dev, symmetric)
    got = _check_rows([[0, 0, 0], [0], [0, -1, 0]], 1, dev, symmetric)     # V = 1
    assert got.counts.tolist() == [8 if symmetric else 4]
    V = 120000                                                             # keys beyond 2^32
    got = _check_rows([[V - 1, V - 2, V - 1, 0], [V - 2, V - 1], [5, V - 1]], V, dev, symmetric)
    assert (V - 1) * V + V - 2 > 2 ** 32 and got.indptr.numel() == V + 1
    assert _check_rows([], 3, dev, symmetric).nnz == 0 and _check_rows([[], []], 3, dev, symmetric).total_windows == 2


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("w", [1, 2, 10])
def test_sliding_windows(dev, symmetric, w):
    rng = np.random.default_rng(20 + w)
    rows = [_random_row(rng, n, 12, oov=0.2) for n in (w - 1, w, w + 1, 3 * w, 0, 3 * w)]
    got = _check_rows(rows, 12, dev, symmetric, window_size=w)
    if w == 1:
        assert got.nnz == 0 and got.total_windows == sum(len(r) for r in rows)    # windows, but no pairs
    _check_rows(rows, 12, dev, symmetric, window_size=w, normalize=True)   # float64 sums in one order: the same bits


def test_chunks_under_max_records_give_the_same_matrix(dev):
    from snx import cooc
    rng = np.random.default_rng(21)
    rows = [_random_row(rng, int(n), 60) for n in rng.integers(0, 30, size=200)]
    rows[77] = _random_row(rng, 400, 60, oov=0.0)                          # alone above the bound: its own chunk
    assert len(set(rows[77])) * (len(set(rows[77])) + 1) // 2 > 1000
    for symmetric in (True, False):
        for normalize in (False, True):
            one = _check_rows(rows, 60, dev, symmetric, normalize=normalize, fast=True)
            many = cooc.cooccurrence(*cooc.id_rows(rows), 60, symmetric=symmetric, normalize=normalize, max_records=1000,
                                     device=dev)
            assert torch.equal(one.indptr, many.indptr) and torch.equal(one.indices, many.indices)
            assert one.data.cpu().numpy().tobytes() == many.data.cpu().numpy().tobytes()
            assert normalize or torch.equal(one.counts, many.counts)


# ------------------------------------------------------------------------------------------------ 4: PMI
def _calculator(g18, dev, i):
    from src.pmi import PMICalculator, PMIConfig
    s = next(x for x in g18["settings"] if x["name"] == g18["pmi_setting"])
    b = _fit(g18, s, dev)
    return PMICalculator(b.device_csr(), b.get_term_frequencies(), b.get_vocabulary(), b.get_stats().total_windows,
                         PMIConfig(**g18["pmi"][i]["config"]), device=dev), b


@pytest.mark.parametrize("i", [0, 1, 2])
def test_pmi_batch_and_matrix_against_the_reference(g18, dev, i):
    calc, b = _calculator(g18, dev, i)
    terms = g18["pmi_terms"]
    pairs = [(x, y) for x in terms for y in terms]
    got = np.array(calc.compute_pmi_batch(pairs, show_progress=False), dtype=np.float64)
    gold = g18["arrays"][f"pmi{i}/batch"]
    assert got.shape == gold.shape
    exact = (gold == 0.0) | np.isinf(gold)                                 # PPMI clamps, OOV, k = 0 below min_cooccurrence
    assert np.array_equal(got[exact], gold[exact]) and exact.any() and not exact.all()
    assert np.isfinite(got[~exact]).all() and (np.sign(got[~exact]) == np.sign(gold[~exact])).all()
    ulps = R.ulps64(got[~exact], gold[~exact])
    print(f"pmi config {i}: largest distance to the reference {int(ulps.max())} float64 ulp over {ulps.size} values")
    assert ulps.max() <= PMI_ULPS
    assert calc.compute_pmi("cat", "dog") == gold[terms.index("cat") * len(terms) + terms.index("dog")]   # host lookup
    m = calc.compute_pmi_matrix()
    data, indices, indptr = (m.data, m.indices, m.indptr) if hasattr(m, "indptr") else m
    c_data, c_indices, c_indptr = b.cooccurrence_csr()
    assert np.array_equal(indices, c_indices) and np.array_equal(indptr, c_indptr) and data.dtype == np.float32
    want = g18["arrays"][f"pmi{i}/matrix"]
    assert np.isfinite(data).all() and np.array_equal(data == 0, want == 0)
    near = np.abs(data.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert near[(data != 0)].max() <= 1 and (np.sign(data) == np.sign(want)).all()


def test_pmi_of_pairs_outside_the_matrix(g18, dev):
    from snx import cooc
    from src.pmi import PMIConfig
    csr = cooc.cooccurrence(*cooc.id_rows([[0, 1]]), 3, device=dev)
    marg = np.array([0.5, 0.5, 0.0])
    for cfg, none in ((PMIConfig(), 0.0), (PMIConfig(use_ppmi=False), -np.inf)):
        out = cooc.pmi_pairs(csr, [-1, 0, -1, 0, 2], [0, -1, -1, 2, 2], marg, 2.0, cfg).cpu().numpy()
        assert out.tolist() == [none] * 5                                  # OOV, and a zero marginal
    empty = cooc.cooccurrence(*cooc.id_rows([[0]]), 2, device=dev)
    out = cooc.pmi_pairs(empty, [0, 1], [1, 1], np.array([0.5, 0.5]), 1.0, PMIConfig(laplace_smoothing=0.0, use_ppmi=False))
    assert out.tolist() == [-np.inf, -np.inf] and cooc.pmi_values(empty, np.array([0.5, 0.5]), 1.0, PMIConfig()).numel() == 0
    with pytest.raises(ValueError):
        cooc.pmi_pairs(csr, [3], [0], marg, 2.0, PMIConfig())
    with pytest.raises(ValueError):
        cooc.pmi_values(csr, marg[:2], 2.0, PMIConfig())


# ------------------------------------------------------------------------------------------------ 5: end to end
def test_pipeline_and_validator_reproduce_the_reference(g18, dev, tmp_path):
    from src.pmi import (CooccurrenceConfig, OOVStrategy, PMIConfig, SynonymValidator, ValidationConfig, WindowType,
                         create_pmi_pipeline)
    s = next(x for x in g18["settings"] if x["name"] == g18["pmi_setting"])
    cooc_config = CooccurrenceConfig(WindowType(s["window_type"]), s["window_size"], s["min_term_freq"],
                                     s["max_vocab_size"], s["symmetric"], s["normalize"])
    for n, v in enumerate(g18["validations"]):
        builder, calc = create_pmi_pipeline(g18["corpus"], cooc_config=cooc_config,
                                            pmi_config=PMIConfig(**g18["pmi"][v["pmi_config"]]["config"]),
                                            save_path=tmp_path / "pmi" if n == 0 else None, show_progress=False, device=dev)
        cfg = ValidationConfig(**{**v["config"], "oov_strategy": OOVStrategy(v["config"]["oov_strategy"])})
        validator = SynonymValidator(calc, cfg)
        validated, result = validator.validate([dict(p) for p in g18["pairs"]], show_progress=False)
        R.check_validation(g18, v, validated, result, validator.thresholds)
    assert os.path.exists(tmp_path / "pmi" / "cooccurrence_matrix.npz")


def test_cli_validates_pairs_and_writes_the_report(g18, dev, tmp_path, capsys):
    import json
    from src.pmi import CooccurrenceConfig, SynonymValidator, create_pmi_pipeline
    from src.train.cli import validate_synonyms as cli
    docs = [d for d in g18["corpus"] if "\n" not in d]                     # the CLI reads one document a line
    (tmp_path / "corpus.txt").write_text("".join(d + "\n" for d in docs), encoding="utf-8")
    (tmp_path / "pairs.json").write_text(json.dumps(g18["pairs"], ensure_ascii=False), encoding="utf-8")
    out = cli.main(["--corpus", str(tmp_path / "corpus.txt"), "--pairs", str(tmp_path / "pairs.json"), "--output-dir",
                    str(tmp_path / "out"), "--min-term-freq", "2", "--device", str(dev)])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == out
    builder, calc = create_pmi_pipeline(docs, cooc_config=CooccurrenceConfig(min_term_freq=2), show_progress=False, device=dev)
    validator = SynonymValidator(calc)
    validated, result = validator.validate([dict(p) for p in g18["pairs"]], show_progress=False)
    assert out["documents"] == len(docs) and out["vocab_size"] == len(builder.get_vocabulary()) > 0
    assert out["total_windows"] == builder.get_stats().total_windows and out["nnz"] == builder.get_stats().total_cooccurrences
    assert (out["total_pairs"], out["valid_pairs"], out["removed_pairs"], out["oov_pairs"]) == \
        (result.total_pairs, result.valid_pairs, result.removed_pairs, result.oov_pairs)
    assert out["thresholds"] == validator.thresholds and 0 < out["valid_pairs"] < out["total_pairs"]
    names = set(os.listdir(tmp_path / "out"))
    assert {"cooccurrence_matrix.npz", "vocabulary.json", "term_frequencies.json", "config.json", "stats.json",
            "validated_pairs.jsonl", "invalid_pairs.jsonl", "validation_report.json"} <= names
    with open(tmp_path / "out" / "validated_pairs.jsonl", encoding="utf-8") as f:
        assert [json.loads(x)["source"] for x in f] == [p.source for p in validated if p.is_valid]
