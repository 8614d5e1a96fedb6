#!/usr/bin/env python3
"""Write tests/golden/g17_tfidf/ by RUNNING the reference's TF-IDF hard-negative miner.

    python tools/make_golden_tfidf.py --reference <checkout of the reference project>

Loads ref:scripts/mine_hard_negatives.py by file path (it needs scikit-learn, scipy and tqdm) and runs its own
``build_corpus``, ``build_tfidf_index``, ``_chunked_topk`` and ``process_shard`` over a seeded corpus generated here.
Data only:

  input/train_shard_00{0,1}.jsonl     the raw shards: about 300 unique positives, Hangul and Latin words and one non-BMP
                                      character, one-character words, mixed case, tabs, newlines and runs of spaces; about
                                      100 records lack a negative (absent, null or ""); a few of those have a positive past
                                      the corpus cap, an empty query or a query of n-grams no document holds; one blank and
                                      one malformed line
  expected/train_shard_00{0,1}.jsonl  what the reference's process_shard wrote
  meta.json                           settings, the feature n-grams in order, the needing records (shard, record index),
                                      the reference's per-shard stats, and the flags of its parse_args() read as text
  arrays.npz                          idf_ float64 [F]; the L2-normalised corpus matrix in float64 as CSR (indptr, indices,
                                      data); scores float64 [needing, corpus] = queries @ corpus.T; nnz_q [needing]; topk
                                      int64 [needing, top_k]: the reference's lists

``max_features`` is chosen below the number of distinct n-grams where the total counts do not tie across the cut (asserted):
among tied n-grams scikit-learn's choice is arbitrary.  Also asserted, on the reference's own float64 scores: wherever the
best and second-best admissible score of a needing record lie more than (nnz_q + 2) * 2^-24 apart, the reference chose
the best admissible document, and records without that gap are at most 5 % of the needing ones."""
import argparse
import importlib.util
import json
import os
import random
import shutil
import sys
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g17_tfidf")
SEED = 1729
MAX_CORPUS = 300
TOP_K = 10
BATCH = 37                             # several batches, the last one short
CHUNK = 128                            # several corpus chunks in the reference's top-k merge

BASE_LATIN = "search engine sparse neural model query document index token weight vector rank score a i o x".split()
BASE_HANGUL = "검색 엔진 희소 신경 모델 질의 문서 색인 토큰 가중치 벡터 순위 점수 서울 부산 한국어 의 는 이 강 돌".split()
SYLLABLES = "가나다라마바사아자차카타파하고노도로모보소오조초코토포호구누두루무부수우주추한글국민서울산강".replace(" ", "")


def make_vocab(rng):
    """The seeded word lists: the base words plus pseudo-words of 2 .. 7 letters and 1 .. 4 Hangul syllables."""
    latin, hangul = list(BASE_LATIN), list(BASE_HANGUL)
    while len(latin) < 170:
        w = "".join(rng.choice("abcdefghijklmnoprstuvwyz") for _ in range(rng.randint(2, 7)))
        if w not in latin:
            latin.append(w)
    while len(hangul) < 170:
        w = "".join(rng.choice(SYLLABLES) for _ in range(rng.randint(1, 4)))
        if w not in hangul:
            hangul.append(w)
    return latin, hangul


EMOJI = "\U0001F600"
GAPS = [" ", " ", " ", "  ", "\t", "\n", "   ", " \t "]


def _case(rng, w):
    r = rng.random()
    return w.upper() if r < 0.1 else w.capitalize() if r < 0.25 else w


def _text(rng, words):
    out = ""
    for i, w in enumerate(words):
        out += (rng.choice(GAPS) if i else "") + _case(rng, w)
    if rng.random() < 0.15:
        out = rng.choice([" ", "\t", "\n"]) + out + rng.choice([" ", "  ", "\n"])
    return out


def _doc(rng, LATIN, HANGUL):
    n = rng.randint(4, 10)
    pool = LATIN if rng.random() < 0.4 else HANGUL if rng.random() < 0.7 else LATIN + HANGUL
    words = [rng.choice(pool) for _ in range(n)]
    if rng.random() < 0.06:
        words[rng.randrange(n)] += EMOJI
    return words


def make_shards(rng):
    LATIN, HANGUL = make_vocab(rng)
    docs, seen = [], set()
    while len(docs) < MAX_CORPUS + 8:                         # the last 8 positives lie past the corpus cap
        w = _doc(rng, LATIN, HANGUL)
        t = _text(rng, w)
        if t not in seen:
            seen.add(t)
            docs.append((w, t))
    records = []
    for i, (w, t) in enumerate(docs):
        for _ in range(2 if rng.random() < 0.07 else 1):
            q = [x for x in w if rng.random() < 0.6] or [w[0]]
            q += [rng.choice(LATIN + HANGUL) for _ in range(rng.randint(0, 2))]
            rng.shuffle(q)
            rec = {"query": _text(rng, q), "positive": t}
            r = rng.random()
            if i >= MAX_CORPUS or r < 0.29:
                if r < 0.1:
                    rec["negative"] = "" if r < 0.05 else None
            else:
                rec["negative"] = docs[rng.randrange(len(docs))][1]
                rec["difficulty"] = rng.choice(["easy", "medium"])
            records.append(rec)
    records[5] = {"query": "", "positive": records[5]["positive"]}                 # an empty query
    records[11] = {"query": " \t\n ", "positive": records[11]["positive"]}         # whitespace only
    records[17] = {"query": "ψψψ ωω ζ", "positive": records[17]["positive"]}       # n-grams no document holds
    records[23] = {"query": "Ψ", "positive": records[23]["positive"], "negative": ""}
    half = len(records) // 2
    return records[:half], records[half:]


def write_shard(path, records, extra_lines):
    with open(path, "w", encoding="utf-8") as f:
        for i, rec in enumerate(records):
            if i in extra_lines:
                f.write(extra_lines[i])
            f.write(json.dumps(rec, ensure_ascii=False) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location(
        "ref_mine_hard_negatives", os.path.join(args.reference, "scripts", "mine_hard_negatives.py"))
    ref = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = ref
    spec.loader.exec_module(ref)
    from sklearn.feature_extraction.text import CountVectorizer
    sys.path.insert(0, ROOT)
    from tests.tfidf_reference import cli_flags_of          # the extractor that the test of the CLI uses, too
    from sklearn.preprocessing import normalize

    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(os.path.join(OUT, "input"))
    os.makedirs(os.path.join(OUT, "expected"))
    rng = random.Random(SEED)
    shards = make_shards(rng)
    names = ["train_shard_000.jsonl", "train_shard_001.jsonl"]
    write_shard(os.path.join(OUT, "input", names[0]), shards[0], {40: "\n", 90: '{"query": "broken", "positive": \n'})
    write_shard(os.path.join(OUT, "input", names[1]), shards[1], {})
    files = [Path(OUT) / "input" / n for n in names]

    corpus = ref.build_corpus(files, MAX_CORPUS)
    assert len(corpus) == MAX_CORPUS
    # the cut: total counts of all n-grams, descending; max_features where the count steps down
    cv = CountVectorizer(analyzer="char_wb", ngram_range=(2, 3))
    totals = np.sort(np.asarray(cv.fit_transform(corpus).sum(axis=0)).ravel())[::-1]
    distinct = int(totals.size)
    max_features = int(distinct * 0.6)
    while max_features > 1 and totals[max_features - 1] == totals[max_features]:
        max_features -= 1
    assert 1 < max_features < distinct and totals[max_features - 1] > totals[max_features], "no tie across the cut"

    vectorizer, corpus_tfidf, corpus = ref.build_tfidf_index(corpus, max_features=max_features)
    features = vectorizer.get_feature_names_out().tolist()
    assert len(features) == max_features

    need, queries, positives = [], [], []
    for s, f in enumerate(files):
        recs = []
        with open(f, encoding="utf-8") as fh:
            for line in fh:
                line = line.strip()
                if not line:
                    continue
                try:
                    recs.append(json.loads(line))
                except json.JSONDecodeError:
                    continue
        for i, rec in enumerate(recs):
            if not rec.get("negative"):
                need.append([s, i])
                queries.append(rec.get("query", ""))
                positives.append(rec.get("positive", ""))
    q_tfidf = normalize(vectorizer.transform(queries), norm="l2", axis=1, copy=False)
    scores = np.asarray((q_tfidf @ corpus_tfidf.T).toarray(), dtype=np.float64)
    nnz_q = np.diff(q_tfidf.indptr).astype(np.int32)
    topk = ref._chunked_topk(q_tfidf, corpus_tfidf, TOP_K, CHUNK)

    stats = [ref.process_shard(shard_file=f, vectorizer=vectorizer, corpus_tfidf=corpus_tfidf, corpus=corpus, top_k=TOP_K,
                               batch_size=BATCH, corpus_chunk_size=CHUNK, output_dir=Path(OUT) / "expected", dry_run=False)
             for f in files]

    # condition 2 of the issue on the reference's own float64 scores
    expected = []
    for n in names:
        with open(os.path.join(OUT, "expected", n), encoding="utf-8") as fh:
            expected.append([json.loads(line) for line in fh])
    doc_of = {t: i for i, t in enumerate(corpus)}
    close = 0
    for r, (s, i) in enumerate(need):
        adm = np.array([t != positives[r] for t in corpus])
        order = np.argsort(-scores[r][adm], kind="stable")
        best = scores[r][adm][order[0]]
        second = scores[r][adm][order[1]]
        tol = (int(nnz_q[r]) + 2) * 2.0 ** -24
        if best - second > tol:
            chosen = expected[s][i].get("negative")
            assert chosen and doc_of[chosen] == int(np.flatnonzero(adm)[order[0]]), (r, chosen)
        else:
            close += 1
    assert close <= 0.05 * len(need), (close, len(need))

    with open(os.path.join(OUT, "meta.json"), "w", encoding="utf-8") as f:
        json.dump({"source": "ref:scripts/mine_hard_negatives.py build_corpus, build_tfidf_index, _chunked_topk, process_shard",
                   "seed": SEED, "ngram_range": [2, 3], "sublinear_tf": True, "max_corpus": MAX_CORPUS,
                   "max_features": max_features, "distinct_ngrams": distinct, "top_k": TOP_K, "batch_size": BATCH,
                   "corpus_chunk_size": CHUNK, "shards": names, "features": features, "need": need, "stats": stats,
                   "close_records": close,
                   "cli_flags": cli_flags_of(os.path.join(args.reference, "scripts", "mine_hard_negatives.py"))}, f, ensure_ascii=False, indent=0)
        f.write("\n")
    ct = corpus_tfidf.tocsr()
    ct.sort_indices()
    np.savez_compressed(os.path.join(OUT, "arrays.npz"), idf=vectorizer.idf_.astype(np.float64),
                        corpus_indptr=ct.indptr.astype(np.int64), corpus_indices=ct.indices.astype(np.int32),
                        corpus_data=ct.data.astype(np.float64), scores=scores, nnz_q=nnz_q, topk=np.asarray(topk, np.int64))
    for n in names:
        os.chmod(os.path.join(OUT, "expected", n), 0o644)
    size = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(OUT) for f in fs)
    print(f"wrote {OUT}: {sum(len(s) for s in shards)} records, {len(need)} needing, corpus {len(corpus)}, "
          f"{max_features} of {distinct} n-grams, {close} close records, stats {stats}, {size} bytes")


if __name__ == "__main__":
    main()
