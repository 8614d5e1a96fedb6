"""Exact sparse retrieval on the GPU (csrc/retrieval.hip, include/snx.h "exact sparse retrieval").

``SparseIndex`` is the inverted index of the mid-training evaluator: the reference hands indexing and search to an
OpenSearch cluster (ref:benchmark/indexer.py, ref:benchmark/searchers.py:155-188); here the doc vectors are packed on the
device batch by batch from the ``[B, cap]`` output of ``ops.sparse_topk`` (no ``[nd, V]`` buffer ever exists), a
term-major index is built by a deterministic counting sort, and every query is scored exactly against every doc:

    s(q, d) = fmaf over the shared terms in ascending term id, fp32, starting at +0  (the plain dot product)

then ranked score descending, ties lowest doc id first.  Results are bit-reproducible and independent of
``chunk_docs``.  ``search_band`` and ``pair_scores`` serve the hard-negative miner (src.train.mining): a rank band of the
ADMISSIBLE docs (score > 0, not in the query's exclusion row, score < the query's ceiling) and s(q, d) of given pairs,
bit-equal to the ranked values.  ``SeismicIndex`` is the approximate SEISMIC search over a built ``SparseIndex``
(csrc/seismic.hip, include/snx.h "SEISMIC").  ``prune_rows``, ``SparseIndex.pruned``, ``SparseIndex.rescore`` and
``SparseIndex.search_two_phase`` are the prune rules and the two-phase search of the reference's ``rank_features``
serving path (csrc/two_phase.hip, include/snx.h "pruning and two-phase search").  ``term_counts``, ``Bm25Index`` and
``fuse_ranked`` are the lexical BM25 baseline under the model's tokenizer and the rank fusion of the reference's hybrid
searchers (csrc/hybrid.hip, include/snx.h "BM25 baseline and rank fusion").  ``relevance_csr``,
``SparseIndex.first_relevant``, ``ranked_relevance`` and ``bootstrap_means`` score any of these searches against qrels with
several relevant docs per query (csrc/qrels.hip, include/snx.h "relevance judgments").  ``DenseIndex`` is the exact
inner-product search over dense fp32 embeddings (csrc/dense.hip, include/snx.h "exact dense retrieval"); its
``search_two_phase`` / ``search_band_two_phase`` return the same result through a bf16 first pass, an exact rescore and a
per-query certificate, on the operands of ``bf16_rows`` (csrc/dense_two_phase.hip, include/snx.h "two-phase dense
retrieval").  ``TfidfIndex`` is
the character n-gram TF-IDF vectorizer of the reference's lexical hard-negative mining over a ``SparseIndex``
(csrc/tfidf.hip, include/snx.h "Character n-gram TF-IDF").  ``IvfFlatIndex`` is the approximate IVF-Flat search over the
same dense embeddings, with ``DenseIndex``'s scores and order inside the probed lists (csrc/ivf.hip, include/snx.h
"IVF-Flat dense retrieval").  ``GraphIndex`` is the approximate graph search over them, a deterministic fixed-degree
graph walked by a best-first beam, again with ``DenseIndex``'s scores and order (csrc/graph.hip, include/snx.h "graph
dense retrieval")."""
from ._common import K_MAX, exclusion_csr
from .dense import DENSE_CHUNK_MIN, DENSE_DIM_MAX, DenseIndex, bf16_rows
from .graph import GRAPH_DEGREE_MAX, GRAPH_EF_MAX, GRAPH_KNN_MAX, GRAPH_WIDTH_MAX, GraphIndex, entry_sample
from .hybrid import (FUSE_L_MAX, FUSE_METHODS, FUSE_TOP_K_MAX, Bm25Index, bm25_idf, fuse_ranked, term_counts,
                     term_counts_max_len)
from .ivf import IVF_NLIST_MAX, IVF_SPLIT_MIN, IvfFlatIndex
from .qrels import (BOOTSTRAP_M_MAX, BOOTSTRAP_SEGMENT, CUTOFFS_MAX, RANKED_R_MAX, bootstrap_indices, bootstrap_means,
                    discount_table, ranked_relevance, relevance_csr)
from .seismic import SEISMIC_Q_MAX, SeismicIndex
from .sparse import CHUNK_MAX, PRUNE_TYPES, WINDOW_MAX, SparseIndex, pack_rows, prune_rows, two_phase_window
from .tfidf import (TfidfIndex, keys_to_ngrams, lds_row_capacity, row_counts, select_features, tfidf_idf, weight_rows,
                    word_rows)
