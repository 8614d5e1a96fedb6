#!/usr/bin/env python3
"""Write tests/golden/g18_pmi/ by RUNNING the reference's src/pmi package (it needs numpy, scipy and tqdm).

    python tools/make_golden_pmi.py --reference <checkout of the reference project>

Loads ref:src/pmi/{cooccurrence,pmi_calculator,synonym_validator}.py by file path and runs CooccurrenceMatrixBuilder,
PMICalculator and SynonymValidator over the corpus below.  Data only:

  g18.json     the corpus; per setting the vocabulary in id order, term_freq, doc_freq and total_windows; the PMI configs
               and the terms their batch covers; the synonym pairs and, per validation config, what ``validate`` returned
  arrays.npz   per setting ``<name>/indptr|indices|data`` of the reference's csr matrix; per PMI config ``pmi<i>/batch``
               (compute_pmi_batch over all pairs of the terms, float64, -inf kept) and ``pmi<i>/matrix`` (the data of
               compute_pmi_matrix, whose structure is the count matrix's)

The corpus covers English and Korean, the four sentence delimiters and the empty line, repeated tokens inside a window, a
token that exists only at document level (``a.b``), an empty and a one-token document, and frequency ties; one setting
cuts the vocabulary inside a tie (asserted).  While writing, the tool asserts that no in-vocabulary pair's score lies
within 1e-9 of the threshold it is compared with, so that a last-bit difference of a logarithm cannot flip a flag."""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g18_pmi")

CORPUS = [
    "the cat sat on the mat. the cat ate the fish! did the dog see the cat? yes",
    "a dog chased the cat\nthe cat ran up the tree",
    "machine learning is fun. deep learning is machine learning",
    "search engines rank documents. a search engine uses an index",
    "neural sparse search uses learned sparse vectors",
    "the index stores sparse vectors\n\nthe engine searches the index\n\n  \n\nvectors are sparse",
    "a.b c a.b",
    "",
    "solo",
    "   ",
    "검색 엔진 은 문서 를 검색 한다. 신경망 검색 은 빠르다",
    "서울 은 대한민국 의 수도 이다! 부산 은 항구 도시 이다",
    "기계 학습 은 재미있다\n\n심층 학습 은 기계 학습 이다",
    "the the the the",
    "cat cat dog dog cat",
    "fish and chips. fish and rice. rice and beans",
    "the dog and the cat are friends? the dog and the fish are not",
    "learning to rank is machine learning for search",
    "sparse vectors and dense vectors. dense vectors are not sparse",
    "an index of documents. an index of vectors",
    "tree tree mat mat",
    "the engine is fast! the search is fast? the index is fast.",
    "검색 검색 검색 엔진 엔진",
    "수도 서울 수도 부산 항구",
    "rank rank rank\n\nrank documents",
    "beans beans chips chips rice",
    "friends are fun. friends are not fish",
    "did the cat see the dog? did the dog see the fish?",
    "one two three four five six seven eight nine ten eleven twelve",
    "one two three four five six seven eight nine ten eleven twelve thirteen",
    "up up down down",
    "yes yes no no",
    "deep neural networks learn. deep networks are neural",
    "networks of neurons\nnetworks of engines",
    "a b c d e f g h i j",
    "j i h g f e d c b a",
    "학습 은 학습 이다. 학습 이다",
    "the mat is on the tree! the tree is on the mat!",
    "documents documents documents index index search",
    "fun fun fun. fun",
    "end of corpus. the end",
]

NO_CUT = 120000
SETTINGS = [
    # window_type, window_size, symmetric, min_term_freq, max_vocab_size, normalize
    ("sentence", 10, True, 1, NO_CUT, False),
    ("sentence", 10, True, 2, NO_CUT, False),
    ("sentence", 10, False, 2, NO_CUT, False),
    ("sentence", 10, True, 5, NO_CUT, False),
    ("sentence", 10, True, 2, None, False),                   # None: a cut inside a frequency tie, chosen below
    ("paragraph", 10, True, 2, NO_CUT, False),
    ("paragraph", 10, False, 1, NO_CUT, False),
    ("sliding", 2, True, 1, NO_CUT, False),
    ("sliding", 3, False, 2, NO_CUT, False),
    ("sliding", 10, True, 5, NO_CUT, False),
    ("sliding", 10, False, 1, NO_CUT, False),
    ("sentence", 10, True, 2, NO_CUT, True),                  # normalised, beside its count twin above
    ("sliding", 3, False, 2, NO_CUT, True),
]
PMI_SETTING = ("sentence", 10, True, 2, NO_CUT, False)
PMI_CONFIGS = [
    dict(laplace_smoothing=1.0, context_smoothing_alpha=0.75, use_ppmi=True, log_base=2.0, min_cooccurrence=1),
    dict(laplace_smoothing=0.0, context_smoothing_alpha=1.0, use_ppmi=False, log_base=float(np.e), min_cooccurrence=1),
    dict(laplace_smoothing=0.1, context_smoothing_alpha=0.75, use_ppmi=False, log_base=10.0, min_cooccurrence=3),
]
OOV_TERMS = ["zebra", "없는단어"]
# (validation config, index of the PMI config it runs on)
VALIDATIONS = [
    (dict(pmi_percentile_threshold=10.0, pmi_absolute_threshold=None, min_embedding_similarity=0.5, oov_strategy="keep",
          separate_bpe_validation=True), 0),
    (dict(pmi_percentile_threshold=34.0, pmi_absolute_threshold=None, min_embedding_similarity=0.5, oov_strategy="remove",
          separate_bpe_validation=False), 1),
    (dict(pmi_percentile_threshold=10.0, pmi_absolute_threshold=0.25, min_embedding_similarity=0.6, oov_strategy="smooth",
          separate_bpe_validation=True), 2),
]
# in-vocabulary pairs of the PMI setting: co-occurring ones, and two that never share a sentence (-inf under config 1)
KNOWN_PAIRS = [
    ("cat", "dog"), ("the", "cat"), ("machine", "learning"), ("sparse", "vectors"), ("search", "engine"),
    ("fish", "rice"), ("검색", "엔진"), ("학습", "기계"), ("수도", "은"), ("index", "documents"), ("deep", "learning"),
    ("the", "mat"), ("tree", "mat"), ("dog", "fish"), ("is", "fun"), ("an", "index"), ("friends", "are"),
    ("neural", "networks"), ("and", "rice"), ("cat", "검색"), ("rank", "fun"),
]
BPE_KNOWN = [("did", "see"), ("dense", "vectors"), ("one", "two"), ("학습", "이다"), ("beans", "chips"), ("on", "mat")]


def name_of(s) -> str:
    wt, w, sym, f, v, norm = s
    return f"{wt}_w{w}_{'sym' if sym else 'asym'}_f{f}_v{v}_{'norm' if norm else 'count'}"


def load_reference(root: str):
    for pkg in ("src", "src.pmi"):
        mod = types.ModuleType(pkg)
        mod.__path__ = []
        sys.modules[pkg] = mod
    mods = {}
    for leaf in ("cooccurrence", "pmi_calculator", "synonym_validator"):
        spec = importlib.util.spec_from_file_location(f"src.pmi.{leaf}", os.path.join(root, "src", "pmi", f"{leaf}.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        mods[leaf] = mod
    return mods["cooccurrence"], mods["pmi_calculator"], mods["synonym_validator"]


def cut_inside_tie(co) -> int:
    """A max_vocab_size that truncates the f >= 2 vocabulary between two terms of one frequency."""
    b = co.CooccurrenceMatrixBuilder(co.CooccurrenceConfig(min_term_freq=2)).fit(CORPUS, show_progress=False)
    tf, terms = b.get_term_frequencies(), list(b.get_vocabulary())
    for cut in range(len(terms) // 2, len(terms)):
        if tf[terms[cut - 1]] == tf[terms[cut]]:
            return cut
    raise AssertionError("the corpus has no frequency tie to cut in")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    co, pc, sv = load_reference(args.reference)
    cut = cut_inside_tie(co)
    settings = [s[:4] + (cut if s[4] is None else s[4],) + s[5:] for s in SETTINGS]
    arrays, recorded, builders = {}, [], {}
    for s in settings:
        wt, w, sym, f, v, norm = s
        cfg = co.CooccurrenceConfig(window_type=co.WindowType(wt), window_size=w, min_term_freq=f, max_vocab_size=v,
                                    symmetric=sym, normalize=norm)
        b = co.CooccurrenceMatrixBuilder(cfg).fit(CORPUS, show_progress=False)
        m = b.get_cooccurrence_matrix()
        m.sort_indices()
        assert m.dtype == np.float32 and (m.data != 0).all()
        name = name_of(s)
        arrays[f"{name}/indptr"] = m.indptr.astype(np.int64)
        arrays[f"{name}/indices"] = m.indices.astype(np.int32)
        arrays[f"{name}/data"] = m.data.astype(np.float32)
        vocab = b.get_vocabulary()
        recorded.append({"name": name, "window_type": wt, "window_size": w, "symmetric": sym, "min_term_freq": f,
                         "max_vocab_size": v, "normalize": norm, "vocab": sorted(vocab, key=vocab.get),
                         "term_freq": b.get_term_frequencies(), "doc_freq": b.get_document_frequencies(),
                         "total_windows": b.get_stats().total_windows, "nnz": int(m.nnz)})
        builders[s] = b
    by_name = {r["name"]: r for r in recorded}
    assert "a.b" in by_name[name_of(settings[1])]["vocab"]        # in the vocabulary, never in a sentence window
    row = by_name[name_of(settings[1])]["vocab"].index("a.b")
    ip = arrays[name_of(settings[1]) + "/indptr"]
    assert ip[row] == ip[row + 1]

    b = builders[PMI_SETTING]
    vocab = b.get_vocabulary()
    terms = sorted(vocab, key=vocab.get) + OOV_TERMS
    all_pairs = [(x, y) for x in terms for y in terms]
    calcs, pmi = [], []
    for i, c in enumerate(PMI_CONFIGS):
        calc = pc.PMICalculator(b.get_cooccurrence_matrix(), b.get_term_frequencies(), vocab,
                                b.get_stats().total_windows, pc.PMIConfig(**c))
        arrays[f"pmi{i}/batch"] = np.array(calc.compute_pmi_batch(all_pairs, show_progress=False), dtype=np.float64)
        pm = calc.compute_pmi_matrix()
        pm.sort_indices()
        count = b.get_cooccurrence_matrix()
        assert np.array_equal(pm.indptr, count.indptr) and np.array_equal(pm.indices, count.indices)
        arrays[f"pmi{i}/matrix"] = pm.data.astype(np.float32)
        calcs.append(calc)
        pmi.append({"config": c})

    for x, y in KNOWN_PAIRS + BPE_KNOWN:
        assert x in vocab and y in vocab, (x, y)
    sims = [0.9, 0.75, 0.55, 0.8, 0.65, 0.95, 0.7, 0.3, 0.85, 0.6, 0.58]
    pairs = []
    for i, (x, y) in enumerate(KNOWN_PAIRS):
        pairs.append({"source": x, "target": y, "similarity": sims[i % len(sims)], "category": "cluster"})
    for i, (x, y) in enumerate(BPE_KNOWN):
        pairs.append({"source": x, "target": y, "similarity": sims[(i + 3) % len(sims)], "category": "BPE"})
    pairs += [
        {"source": "zebra", "target": "cat", "similarity": 0.9, "category": "cluster"},
        {"source": "cat", "target": "zebra", "similarity": 0.8, "category": "cluster"},
        {"source": "zebra", "target": "없는단어", "similarity": 0.7, "category": "cluster"},
        {"source": "cat", "target": "없는단어", "similarity": 0.2, "category": "cluster"},
        {"source": "##ing", "target": "learning", "similarity": 0.9, "category": "BPE"},
        {"source": "learn", "target": "##ing", "similarity": 0.4, "category": "BPE"},
        {"source": "dog", "target": "cat"},                      # no similarity, no category: the defaults
    ]
    validations = []
    for vcfg, pi in VALIDATIONS:
        cfg = sv.ValidationConfig(**{**vcfg, "oov_strategy": sv.OOVStrategy(vcfg["oov_strategy"])})
        validated, result = sv.SynonymValidator(calcs[pi], cfg).validate([dict(p) for p in pairs], show_progress=False)
        # the thresholds the reference compared with (it does not record them): recomputed from the scores it returned
        groups = {"all": validated}
        if cfg.separate_bpe_validation:
            groups = {"cluster": [p for p in validated if p.category != "BPE"],
                      "BPE": [p for p in validated if p.category == "BPE"]}
        thresholds = {}
        for g, members in groups.items():
            raw = calcs[pi].compute_pmi_batch([(p.source, p.target) for p in members], show_progress=False)
            known = [s for p, s in zip(members, raw) if p.oov_status == "both_in_vocab" and not np.isinf(s)]
            if cfg.pmi_absolute_threshold is not None:
                t = cfg.pmi_absolute_threshold
            else:
                t = float(np.percentile(known, cfg.pmi_percentile_threshold)) if known else 0.0
            thresholds[g] = t
            near = [s for s in known if abs(s - t) <= 1e-9]
            assert not near, f"validation {vcfg}: scores {near} lie within 1e-9 of the threshold {t} of batch {g}"
        validations.append({
            "config": vcfg, "pmi_config": pi, "thresholds": thresholds,
            "pairs": [{"source": p.source, "target": p.target, "category": p.category, "oov_status": p.oov_status,
                       "is_valid": bool(p.is_valid), "embedding_similarity": float(p.embedding_similarity),
                       "pmi_score": repr(float(p.pmi_score))} for p in validated],
            "result": {"total_pairs": result.total_pairs, "valid_pairs": result.valid_pairs,
                       "removed_pairs": result.removed_pairs, "oov_pairs": result.oov_pairs,
                       "pmi_threshold": result.pmi_threshold, "stats": result.stats}})
        statuses = {p.oov_status for p in validated}
        assert statuses == {"both_in_vocab", "source_oov", "target_oov", "both_oov"}

    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "g18.json"), "w", encoding="utf-8") as f:
        json.dump({"source": "ref:src/pmi CooccurrenceMatrixBuilder, PMICalculator, SynonymValidator",
                   "corpus": CORPUS, "cut": cut, "settings": recorded, "pmi_setting": name_of(PMI_SETTING),
                   "pmi_terms": terms, "pmi": pmi, "pairs": pairs, "validations": validations}, f, ensure_ascii=False,
                  indent=1)
        f.write("\n")
    np.savez_compressed(os.path.join(OUT, "arrays.npz"), **arrays)
    print(f"wrote {OUT}: {len(CORPUS)} documents, {len(recorded)} settings (cut {cut}), |V| of the PMI setting "
          f"{len(vocab)}, {len(pairs)} pairs")


if __name__ == "__main__":
    main()
