#!/usr/bin/env python3
"""Write tests/golden/g25_mlm_data/ by RUNNING the pure functions of the reference's MLM data script.

    python tools/make_golden_mlm_data.py --reference <checkout of the reference project>

Loads ref:scripts/prepare_korean_mlm_data.py by file path and calls only ``clean_text``, ``split_paragraphs``,
``is_valid_paragraph``, ``korean_ratio``, ``text_hash``, ``deduplicate``, ``split_train_val`` and ``save_lines``; it never
calls ``load_dataset`` (``datasets`` and ``tqdm`` are stubbed when they do not import).  Data only, gzipped JSON:

  cases.json.gz     edge documents and 300 seeded random documents of 0 .. 400 code points over an alphabet of blanks, LF,
                    CR, VT, FF, U+001C, U+0085, U+00A0, U+3000, U+2028, U+200B, Hangul at both ends of the reference's range
                    and just outside, ASCII and an astral code point; per document and per (min_length, ratio) of GRID the
                    paragraph list of clean_text -> split_paragraphs -> is_valid_paragraph
  pipeline.json.gz  two runs of the whole chain over two sources with duplicates inside a document, across documents and
                    across sources: the valid paragraphs, their text_hash, the deduplicated list, train, val, the SHA-256
                    and size of the two written files, and the statistics of print_stats as floats.  Run "main": val_ratio
                    0.05, seed 42.  Run "single": one unique paragraph, where int(n * 0.95) == 0."""
import argparse
import gzip
import hashlib
import importlib.util
import json
import os
import random
import sys
import tempfile
import types
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g25_mlm_data")
GRID = [(0, 0.0), (1, 0.1), (3, 0.3), (5, 1 / 3), (2, 0.5), (1, 1.0), (50, 0.3)]

EDGE = [
    "", " ", "\n", "가", "a", " \t \u3000\n\n \r\n", "가 \t  나", "\t가", "가\t\t나", "가\n나", "가\n\n나", "가\n\n\n나",
    "가\n\n\n\n나", "가\n\n\n\n\n\n\n나", "가\n \n나", "가\r\n\r\n나", "\n\n가", "가\n\n", "\n가\n", " 가 \n\n 나 ",
    "가\u3000 \n", "\u3000가\u3000\n\n\u3000나\u3000", "가 \n\n\n 나\n\n다", "가\x0b\n\n\x0c나", "\x1c가\x1f\n\n\x85나\xa0",
    "\u2028가\u2029", "\u200b가\u200b\n\n\u200b", "가\n\n \n\n나", "가\n\n\t\n\n\n나", "\uabff가힣\ud7af\ud7b0",
    "abcdefghi가", "abcdefghijklmnopqrs가나", "가" * 3 + "a" * 27, "\U0001f600 가 \U0001f600", "a  \t\t  b",
    "가나다라마바사 " * 12 + "\n\n" + "가나다라마바사 " * 12, "x\n\n\n\ny\n\n\nz\n\nw\nv",
]

ALPHABET = ([" "] * 6 + ["\t"] * 3 + ["\n"] * 8 + ["\r", "\x0b", "\x0c", "\x1c", "\x85", "\xa0", "\u3000", "\u2028", "\u200b",
            "\uabff", "\ud7b0", "\U0001f600"] + ["가", "힣", "\ud7af", "한", "글"] * 3 + list("abcXYZ019.,"))


def load_reference(reference: str):
    for name in ("datasets", "tqdm"):
        try:
            __import__(name)
        except Exception:
            stub = types.ModuleType(name)
            stub.load_dataset = None
            stub.tqdm = lambda it, **kw: it
            sys.modules[name] = stub
    spec = importlib.util.spec_from_file_location("ref_prepare_korean_mlm_data",
                                                  os.path.join(reference, "scripts", "prepare_korean_mlm_data.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    mod.tqdm = lambda it, **kw: it                           # no progress bars in a tool's output
    return mod


def paragraphs_of(mod, doc: str, min_length: int, ratio: float):
    text = mod.clean_text(doc)
    if not text:
        return []
    return [p for p in mod.split_paragraphs(text) if mod.is_valid_paragraph(p, min_length, ratio)]


def korean_paragraph(rng: random.Random, words: int) -> str:
    out = []
    for _ in range(words):
        if rng.random() < 0.2:
            out.append("".join(rng.choice("abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(rng.randint(1, 8))))
        else:
            out.append("".join(chr(rng.randint(0xAC00, 0xD7A3)) for _ in range(rng.randint(1, 6))))
    return " ".join(out)


def pipeline_sources(rng: random.Random):
    pool = [korean_paragraph(rng, rng.randint(12, 40)) for _ in range(48)]
    pool[3] = pool[3][:30] + "\n" + pool[3][30:]             # a single LF inside: hashed with it, written as a space
    pool[4] = pool[4][:25] + "\r" + pool[4][25:]             # CR and U+2028 are written as they are
    pool[5] = pool[5][:25] + "\u2028" + pool[5][25:]
    pool[6] = pool[6].replace(" ", "  \t ", 3)               # cleaned to single spaces: equals nothing else
    short = "짧은 문단"                                       # below min_length
    latin = "this paragraph is long enough but holds no hangul at all, so the ratio test drops it"
    wiki, mc4 = [], []
    for d in range(14):
        parts = [pool[(3 * d + k) % 40] for k in range(4)]
        if d % 3 == 0:
            parts.append(parts[0])                           # a duplicate inside the document
        if d % 4 == 1:
            parts.insert(1, short)
        if d % 5 == 2:
            parts.insert(2, latin)
        wiki.append(("\n\n\n" if d % 2 else "\n\n").join(parts) + ("\n" if d % 2 else ""))
    wiki.insert(5, "")
    wiki.insert(9, " \n\n \t\n")
    for d in range(10):
        parts = [pool[(5 * d + k) % 48] for k in range(3)]   # rows 40..47 appear here only; the rest repeat the wiki's
        mc4.append("  " + "\n\n".join(parts) + "  ")
    mc4.append(pool[6].replace("  \t ", " "))                # equals wiki's pool[6] AFTER cleaning: a cross-source duplicate
    return [wiki, mc4]


def run_pipeline(mod, sources, min_length, ratio, val_ratio, seed):
    valid = [p for docs in sources for d in docs for p in paragraphs_of(mod, d, min_length, ratio)]
    unique = mod.deduplicate(valid)
    train, val = mod.split_train_val(unique, val_ratio=val_ratio, seed=seed)
    files = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, rows in (("train", train), ("val", val)):
            path = Path(tmp) / f"{name}.txt"
            mod.save_lines(rows, path)
            data = path.read_bytes()
            files[name] = {"sha256": hashlib.sha256(data).hexdigest(), "bytes": len(data)}
    total = len(train) + len(val)
    every = train + val
    stats = {"total": total, "train": len(train), "val": len(val),
             "mean_length": sum(len(p) for p in every) / total if total else 0,
             "mean_korean_ratio": sum(mod.korean_ratio(p) for p in every) / total if total else 0}
    return {"sources": sources, "min_length": min_length, "min_korean_ratio": ratio, "val_ratio": val_ratio, "seed": seed,
            "valid": valid, "valid_sha256": [mod.text_hash(p) for p in valid], "unique": unique, "train": train,
            "val": val, "files": files, "stats": stats}


def dump(name: str, obj) -> int:
    data = json.dumps(obj, ensure_ascii=True, indent=None, separators=(",", ":")).encode("ascii")
    path = os.path.join(OUT, name)
    with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
        g.write(data)
    return os.path.getsize(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    mod = load_reference(args.reference)
    rng = random.Random(25)
    docs = list(EDGE)
    for _ in range(300):
        docs.append("".join(rng.choice(ALPHABET) for _ in range(rng.randint(0, 400))))
    cases = {"source": "ref:scripts/prepare_korean_mlm_data.py clean_text, split_paragraphs, is_valid_paragraph",
             "grid": [list(g) for g in GRID], "documents": docs,
             "paragraphs": [[paragraphs_of(mod, d, m, r) for d in docs] for m, r in GRID],
             "known_sha256": {"": mod.text_hash(""), "가\n나": mod.text_hash("가\n나")}}
    os.makedirs(OUT, exist_ok=True)
    size_c = dump("cases.json.gz", cases)
    sources = pipeline_sources(random.Random(26))
    single = [["가나다라마 바사아자차 카타파하 " * 4 + "\n\n" + "short"], ["  " + "가나다라마 바사아자차 카타파하 " * 4]]
    pipe = {"source": "ref:scripts/prepare_korean_mlm_data.py deduplicate, split_train_val, save_lines, print_stats",
            "main": run_pipeline(mod, sources, 50, 0.3, 0.05, 42),
            "single": run_pipeline(mod, single, 50, 0.3, 0.05, 42)}
    size_p = dump("pipeline.json.gz", pipe)
    m, s = pipe["main"], pipe["single"]
    print(f"wrote {OUT}: cases.json.gz {size_c} bytes ({len(docs)} documents x {len(GRID)} settings), pipeline.json.gz "
          f"{size_p} bytes (main: {len(m['valid'])} valid, {len(m['unique'])} unique, {len(m['train'])} train, "
          f"{len(m['val'])} val; single: {len(s['unique'])} unique, {len(s['train'])} train, {len(s['val'])} val)")


if __name__ == "__main__":
    main()
