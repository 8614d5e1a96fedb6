#!/usr/bin/env python3
"""The Unigram tokenizer on the GPU (snx.unigram) next to the `tokenizers` library on the same box, and the dense teacher
fed by it.  The protocol of tools/gpu_tokenizer_bench.py.

    python tools/gpu_unigram_bench.py [--fixture TOKENIZER_DIR] [--docs 100000] [--queries 100000] [--repeats 3]
                                      [--batch 100000] [--threads 16] [--teacher-texts 2000]

Synthetic Korean / Latin text drawn from the vocabulary of ``--fixture`` (a directory with tokenizer.json; by default the
test fixture, unpacked from tests/golden/g24_unigram): documents of about 256 tokens, queries of about 16 (word-initial
pieces joined by spaces, a word-internal piece glued on now and then, some punctuation).  No row holds a joining code
point or added-token text, so ``host_rows`` is 0: natural text with combining marks or decomposed Hangul pays the host
restatement for those rows, which this tool does not measure.
Per size, after one warm-up run, ``--repeats`` runs of ``encode_rows`` over batches of ``--batch`` texts; a run's ``pack``
is the sum of the calls' ``last_stats["pack_s"]`` (the host-row test, the code-point CSR), its ``device`` the sum of
``device_s`` (upload, normalize, pieces, fill, the scans, two host reads) and ``both`` the wall time of the loop.  Where
`tokenizers` imports, ``encode_batch`` of the same texts with RAYON_NUM_THREADS = ``--threads`` is timed in the same loop,
the two sides taking turns, and the ids of the first thousand texts are compared.  One JSON line per size: texts/s and
tokens/s of every part from the median run, and median / minimum / maximum seconds.
Then one line for ``TeacherEncoder.encode`` at BGE-M3's geometry with random weights (24 layers, 1024 wide; the fixture's
vocabulary) over ``--teacher-texts`` documents at max_length 256: the list path (the host restatement's ids as Python
lists, padded tensors per batch) against the CSR path (ids stay on the device), interleaved; the embeddings must be
bit-equal.  Nothing is asserted about speed."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "opensearch-neural-pre-train_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

META = "\N{LOWER ONE EIGHTH BLOCK}"


def word_lists(fixture: str):
    with open(os.path.join(fixture, "tokenizer.json"), encoding="utf-8") as f:
        vocab = [p for p, _ in json.load(f)["model"]["vocab"]]
    letters = lambda w: w and all(ch.isalpha() for ch in w)                               # noqa: E731
    first = [w[1:] for w in vocab if w.startswith(META) and letters(w[1:])]
    inner = [w for w in vocab if letters(w)]
    return first, inner


def sentences(count: int, first, inner, seed: int):
    """``count`` sentences of about 16 tokens."""
    r = random.Random(seed)
    out = []
    for _ in range(count):
        want = max(1, int(r.gauss(16, 2)))
        words, k = [], 0
        while k < want:
            w = r.choice(first)
            k += 1
            if r.random() < 0.3:
                w += r.choice(inner)
                k += 1
            if r.random() < 0.08:
                w += r.choice(".,?!")
                k += 1
            words.append(w)
        out.append(" ".join(words))
    return out


def synth(n: int, tokens: int, pool, seed: int):
    """``n`` texts of ``tokens // 16`` sentences of the pool each."""
    r = random.Random(seed)
    k = max(1, tokens // 16)
    return [" ".join(r.choices(pool, k=k)) for _ in range(n)]


def summary(runs):
    return {"median_s": round(statistics.median(runs), 4), "min_s": round(min(runs), 4), "max_s": round(max(runs), 4)}


def rates(n_texts: int, n_tokens: int, seconds: float):
    return {"texts_per_s": round(n_texts / seconds), "tokens_per_s": round(n_tokens / seconds)} if seconds > 0 else {}


def teacher_row(tok, fixture: str, texts, repeats: int):
    import torch
    from snx.teacher import TeacherConfig, TeacherEncoder, random_state_dict
    from snx.unigram import UnigramTokenizer
    cfg = TeacherConfig(vocab_size=len(tok), max_position_embeddings=514)
    enc = TeacherEncoder(cfg, random_state_dict(cfg, 3), device="cuda", precision="bf16")
    host = UnigramTokenizer.from_pretrained(fixture, device="cpu")
    parts = {"list_path": [], "csr_path": []}
    equal = True
    for it in range(repeats + 1):
        out = {}
        for name, t in (("list_path", host), ("csr_path", tok)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[name] = enc.encode(texts, t, max_length=256)
            torch.cuda.synchronize()
            if it:
                parts[name].append(time.perf_counter() - t0)
        equal = equal and bool(torch.equal(out["list_path"], out["csr_path"]))
    line = {"bench": "gpu_unigram_teacher", "texts": len(texts), "max_length": 256, "layers": cfg.num_hidden_layers,
            "hidden": cfg.hidden_size, "precision": "bf16", "repeats": repeats, "bit_equal": equal}
    for k, runs in parts.items():
        line[k] = {**summary(runs), "texts_per_s": round(len(texts) / statistics.median(runs))}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixture", default=None)
    ap.add_argument("--docs", default="100000")
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=100000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--teacher-texts", type=int, default=2000, help="0: no teacher row")
    args = ap.parse_args()
    if args.fixture is None:
        from tests.unigram_reference import fixture_dir
        args.fixture = fixture_dir()
    os.environ.setdefault("RAYON_NUM_THREADS", str(args.threads))
    os.environ.setdefault("TOKENIZERS_PARALLELISM", "true")
    import torch
    from snx.unigram import UnigramTokenizer
    tok = UnigramTokenizer.from_pretrained(args.fixture, device="cuda")
    try:
        from tokenizers import Tokenizer
        lib = Tokenizer.from_file(os.path.join(args.fixture, "tokenizer.json"))
        lib.no_truncation()
    except ImportError:
        lib = None
    first, inner = word_lists(args.fixture)
    pool = sentences(50000, first, inner, seed=1)
    sizes = [("docs", int(n), 256) for n in args.docs.split(",") if n] + [("queries", args.queries, 16)]
    for kind, n, tokens in sizes:
        texts = synth(n, tokens, pool, seed=n + tokens)
        batches = [texts[b:b + args.batch] for b in range(0, n, args.batch)]
        parts = {"pack": [], "device": [], "both": [], "library": []}
        n_tokens, same, host_rows = 0, None, 0
        if lib is not None:                                       # the ids of the first thousand texts, both sides
            p, ids = tok.encode_rows(texts[:1000])
            p, flat = p.tolist(), ids.tolist()
            same = all(flat[p[r]:p[r + 1]] == e.ids for r, e in enumerate(lib.encode_batch(texts[:1000])))
        for it in range(args.repeats + 1):
            pack = device = 0.0
            n_tokens = host_rows = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in batches:
                _, ids = tok.encode_rows(b)
                pack += tok.last_stats["pack_s"]
                device += tok.last_stats["device_s"]
                host_rows += tok.last_stats["host_rows"]
                n_tokens += int(ids.numel()) - 2 * len(b)
            both = time.perf_counter() - t0
            lib_s = None
            if lib is not None:                                   # the two sides take turns
                t0 = time.perf_counter()
                for b in batches:
                    lib.encode_batch(b)
                lib_s = time.perf_counter() - t0
            print(f"# {kind} {n}: run {it}: both {both:.2f} s" + ("" if lib_s is None else f", library {lib_s:.2f} s"),
                  file=sys.stderr, flush=True)
            if it:                                                # run 0 warms up
                for k, v in (("pack", pack), ("device", device), ("both", both), ("library", lib_s)):
                    if v is not None:
                        parts[k].append(v)
        line = {"bench": "gpu_unigram", "kind": kind, "texts": n, "tokens": n_tokens, "tokens_per_text": round(n_tokens / n, 1),
                "batch": args.batch, "repeats": args.repeats, "host_rows": host_rows}
        for k, runs in parts.items():
            if runs:
                line[k] = {**summary(runs), **rates(n, n_tokens, statistics.median(runs))}
        if lib is not None:
            line["library_threads"] = int(os.environ["RAYON_NUM_THREADS"])
            line["first_1000_equal"] = same
        print(json.dumps(line), flush=True)
    if args.teacher_texts > 0:
        teacher_row(tok, args.fixture, synth(args.teacher_texts, 256, pool, seed=7), args.repeats)


if __name__ == "__main__":
    main()
