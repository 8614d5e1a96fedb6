"""Plain numpy BM25: the tests' reference for snx_term_counts, snx_bm25_doc_freq and snx_bm25_weights (csrc/hybrid.hip; the
definition: include/snx.h "BM25 baseline and rank fusion").

The weights are np.float64 arithmetic with one rounded operation per numpy call, in the contract's order, then one
rounding to fp32 -- what the kernel computes bit for bit.  The idf table is the same host numpy call on both sides."""
import numpy as np


def term_counts(input_ids, attention_mask, allowed):
    """-> (term [n, S] int32 ascending distinct counted ids, unused -1; tf [n, S] int32, unused 0; cnt [n]; length [n])."""
    ids, mask, allowed = np.asarray(input_ids, np.int64), np.asarray(attention_mask), np.asarray(allowed)
    n, S = ids.shape
    V = len(allowed)
    term, tf = np.full((n, S), -1, np.int32), np.zeros((n, S), np.int32)
    cnt, length = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for r in range(n):
        ok = (mask[r] != 0) & (ids[r] >= 0) & (ids[r] < V)
        ok[ok] = allowed[ids[r][ok]] != 0
        u, c = np.unique(ids[r][ok], return_counts=True)
        term[r, :len(u)], tf[r, :len(u)], cnt[r], length[r] = u, c, len(u), int(ok.sum())
    return term, tf, cnt, length


def rows_of(term, tf, cnt):
    return [(term[r, :c].astype(np.int64), tf[r, :c].astype(np.int64)) for r, c in enumerate(cnt)]


def doc_freq(rows, V):
    df = np.zeros(V, np.int64)
    for t, _ in rows:
        df[t] += 1
    return df


def idf(df, N):
    df = np.asarray(df, np.float64)
    return np.log1p((np.float64(N) - df + 0.5) / (df + 0.5))


def avgdl(dl):
    dl = np.asarray(dl, np.int64)
    return float(np.float64(int(dl.sum())) / np.float64(len(dl))) if len(dl) else 0.0


def weights(rows, dl, idf_table, avg, k1=1.2, b=0.75):
    """rows: (terms, tf) per doc -> fp32 weight rows: (float)(idf * (tf / (tf + k1 * ((1 - b) + b * (dl / avgdl)))))."""
    k1, b, avg = np.float64(k1), np.float64(b), np.float64(avg)
    out = []
    for (t, f), n in zip(rows, dl):
        f = np.asarray(f, np.float64)
        norm = k1 * ((np.float64(1.0) - b) + b * (np.float64(n) / avg)) if len(f) else np.float64(0)
        out.append((np.asarray(t, np.int64), (np.asarray(idf_table, np.float64)[t] * (f / (f + norm))).astype(np.float32)))
    return out


def bm25_rows(input_ids, attention_mask, allowed, k1=1.2, b=0.75):
    """Tokenized docs -> (weight rows, df, dl, idf, avgdl)."""
    term, tf, cnt, length = term_counts(input_ids, attention_mask, allowed)
    rows = rows_of(term, tf, cnt)
    df = doc_freq(rows, len(allowed))
    table = idf(df, len(rows))
    avg = avgdl(length)
    return weights(rows, length, table, avg, k1, b), df, length, table, avg


def query_rows(input_ids, attention_mask, allowed):
    term, tf, cnt, _ = term_counts(input_ids, attention_mask, allowed)
    return [(t, f.astype(np.float32)) for t, f in rows_of(term, tf, cnt)]
