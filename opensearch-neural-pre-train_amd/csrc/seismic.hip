// SEISMIC approximate sparse retrieval (Bruch, Nardini, Rulli, Venturini, SIGIR 2024) over the exact index of
// retrieval.hip: the ANN method the reference deploys into an OpenSearch `sparse_vector` field
// (ref:huggingface/v33/README.md; ref:benchmark/searchers.py:130) and measures at ref:scripts/neural_sparse_search_aws.py
// :1314-1510.  The contract (include/snx.h "SEISMIC") is a deterministic form of the published algorithm; it does not claim
// OpenSearch's numbers (no centroid sampling, fp32 summaries without quantization, one index per corpus).
//
// Build, from the term-major lists of snx_sparse_index_build (every list in doc order) and the doc CSR:
//   sz_prune_kernel     one workgroup per term: an 8-bit radix select on the weight bits keeps the n_postings heaviest
//                       postings (ties: lowest doc id), written in doc order by an ordered ballot compaction;
//   sz_centroid_kernel  one workgroup per term: the rank of every kept posting under (weight desc, doc asc) by counting
//                       (keys tiled through LDS; O(p^2 / 256) per term, p <= n_postings); rank floor(j p / c) is centroid j;
//   sz_assign_kernel    one workgroup per term, one lane per kept posting, the centroids' rows staged in LDS: the centroid
//                       of highest s(doc, centroid) (full doc vectors, the ABI dot product, ties lowest j) and an integer
//                       count per centroid;
//   sz_fill_kernel      one workgroup per term: the stable counting sort of the kept postings by centroid, 256 postings
//                       per step, from the block cursors the host scanned out of the counts (empty blocks occupy nothing);
//   sz_summary_kernel   a fixed grid of workgroups, each owning one slot of the caller's workspace ([V] max table, [V]
//                       term list, [pow2 >= V] sort buffer) and walking blocks slot, slot + G, ...: the union of the
//                       block's doc vectors by an integer max on the fp32 bits (weights > 0: order-independent), a bitonic
//                       sort by (m desc, u asc) in LDS (in the slot when the union has more than SZ_SORT_LDS terms), the
//                       fp32 left folds on one lane, then the kept prefix in ascending term id.  A count pass and a fill
//                       pass around the host's scan of the counts; the touched table entries are reset after each block.
// Search (sz_search_kernel): one workgroup per query.  The query (sorted by term) and its top_n cut live in LDS; per cut
// term the summary scores of up to 256 blocks are computed at once (one lane per block), then the blocks are walked in
// order against the running k-th score; a scored block's docs are scored one lane per doc (merge walk against the query,
// fmaf chain) and merged into the sorted top k in LDS (64-bit keys score bits << 32 | ~doc, double-buffered, every key
// placed by counting, so the result depends on the key set only).  No float atomics: byte-identical from run to run.
// row_dot, the rank key (score bits << 32 | ~doc) and bitonic_desc come from sparse_common.h.
#include "sparse_common.h"
#include "snx.h"

namespace {

constexpr int SZ_THREADS = 256;
constexpr int SZ_WAVES = SZ_THREADS / 64;
constexpr int SZ_QMAX = 1024;                    // query nnz cap of the search (LDS)
constexpr int SZ_KMAX = 1024;
constexpr int SZ_SORT_LDS = 4096;                // summary unions up to this size sort in LDS, larger ones in the slot
constexpr int SZ_SLOTS = 256;                    // summary workgroups (workspace slots)
constexpr int SZ_RTILE = 1024;                   // rank-by-counting tile
constexpr int SZ_CTILE = 512;                    // centroid rows staged per step of the assignment

// ------------------------------------------------------------------------------------------------ build: pruning
__global__ __launch_bounds__(SZ_THREADS) void sz_prune_kernel(const int64_t* __restrict__ term_ptr,
                                                              const int32_t* __restrict__ post_doc,
                                                              const float* __restrict__ post_w, int32_t n_postings,
                                                              const int64_t* __restrict__ prune_ptr,
                                                              int32_t* __restrict__ prune_doc,
                                                              float* __restrict__ prune_w) {
  __shared__ int hist[256];
  __shared__ int sh[2];
  __shared__ int wcnt[2][SZ_WAVES];
  __shared__ int run[2];
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t a = term_ptr[t], L = term_ptr[t + 1] - a, out0 = prune_ptr[t];
  const bool select = L > n_postings;
  uint32_t thr = 0u;
  int need_eq = 0;
  if (select) {                                              // the n_postings largest weight bit patterns
    uint32_t prefix = 0u, known = 0u;
    int remaining = n_postings;
    for (int shift = 24; shift >= 0; shift -= 8) {
      for (int i = tid; i < 256; i += SZ_THREADS) hist[i] = 0;
      __syncthreads();
      for (int64_t i = tid; i < L; i += SZ_THREADS) {
        const uint32_t kk = fbits(post_w[a + i]);
        if ((kk & known) == prefix) atomicAdd(&hist[(kk >> shift) & 255u], 1);
      }
      __syncthreads();
      if (tid == 0) {
        int rem = remaining, b = 255;
        for (; b > 0; --b) {
          if (hist[b] >= rem) break;
          rem -= hist[b];
        }
        sh[0] = b;
        sh[1] = rem;
      }
      __syncthreads();
      prefix |= (uint32_t)sh[0] << shift;
      known |= 255u << shift;
      remaining = sh[1];
      __syncthreads();
    }
    thr = prefix;
    need_eq = remaining;
  }
  // ordered compaction in list (= doc) order: every key > thr and the first need_eq keys == thr (everything when L fits)
  const unsigned long long below = (1ull << lane) - 1ull;
  if (tid == 0) { run[0] = 0; run[1] = 0; }
  __syncthreads();
  for (int64_t base = 0; base < L; base += SZ_THREADS) {
    const int64_t i = base + tid;
    const uint32_t kk = i < L ? fbits(post_w[a + i]) : 0u;
    const bool gt = i < L && (!select || kk > thr);
    const bool eq = i < L && select && kk == thr;
    const unsigned long long mg = __ballot(gt), me = __ballot(eq);
    if (lane == 0) { wcnt[0][wave] = __popcll(mg); wcnt[1][wave] = __popcll(me); }
    __syncthreads();
    int E = run[0], T = run[1];
    for (int w = 0; w < wave; ++w) {
      T += wcnt[0][w] + min(max(need_eq - E, 0), wcnt[1][w]);
      E += wcnt[1][w];
    }
    const int eq_below = __popcll(me & below);
    if (gt || (eq && E + eq_below < need_eq)) {
      const int pos = T + __popcll(mg & below) + min(max(need_eq - E, 0), eq_below);
      prune_doc[out0 + pos] = post_doc[a + i];
      prune_w[out0 + pos] = post_w[a + i];
    }
    __syncthreads();
    if (tid == 0) {
      int e = run[0], tt = run[1];
      for (int w = 0; w < SZ_WAVES; ++w) {
        tt += wcnt[0][w] + min(max(need_eq - e, 0), wcnt[1][w]);
        e += wcnt[1][w];
      }
      run[0] = e;
      run[1] = tt;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ build: centroids
// rank under (weight desc, doc asc) = #{greater keys}, key = weight bits << 32 | ~doc (distinct within a list)
__global__ __launch_bounds__(SZ_THREADS) void sz_centroid_kernel(const int64_t* __restrict__ prune_ptr,
                                                                 const int32_t* __restrict__ prune_doc,
                                                                 const float* __restrict__ prune_w,
                                                                 const int32_t* __restrict__ cent_cnt,
                                                                 const int64_t* __restrict__ cent_ptr,
                                                                 int32_t* __restrict__ cent_doc) {
  __shared__ unsigned long long tile[SZ_RTILE];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int64_t a = prune_ptr[t], p = prune_ptr[t + 1] - a;
  const int64_t c = cent_cnt[t], c0 = cent_ptr[t];
  if (p <= 0 || c <= 0) return;                              // uniform over the workgroup
  for (int64_t base = 0; base < p; base += SZ_THREADS) {
    const int64_t i = base + tid;
    const unsigned long long ki = i < p ? rank_key(fbits(prune_w[a + i]), (uint32_t)prune_doc[a + i]) : 0ull;
    int64_t rank = 0;
    for (int64_t j0 = 0; j0 < p; j0 += SZ_RTILE) {
      const int n = (int)min((int64_t)SZ_RTILE, p - j0);
      for (int j = tid; j < n; j += SZ_THREADS)
        tile[j] = rank_key(fbits(prune_w[a + j0 + j]), (uint32_t)prune_doc[a + j0 + j]);
      __syncthreads();
      for (int j = 0; j < n; ++j) rank += tile[j] > ki;
      __syncthreads();
    }
    if (i < p) {                                             // centroid j sits at rank floor(j p / c): j = ceil(rank c / p)
      const int64_t j = (rank * c + p - 1) / p;
      if (j < c && (j * p) / c == rank) cent_doc[c0 + j] = prune_doc[a + i];
    }
  }
}

__global__ __launch_bounds__(SZ_THREADS) void sz_assign_kernel(const int64_t* __restrict__ prune_ptr,
                                                               const int32_t* __restrict__ prune_doc,
                                                               const int32_t* __restrict__ cent_cnt,
                                                               const int64_t* __restrict__ cent_ptr,
                                                               const int32_t* __restrict__ cent_doc,
                                                               const int64_t* __restrict__ doc_ptr,
                                                               const int32_t* __restrict__ doc_term,
                                                               const float* __restrict__ doc_w,
                                                               int32_t* __restrict__ assign,
                                                               int32_t* __restrict__ cent_size) {
  __shared__ int64_t crow[2][SZ_CTILE];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int64_t a = prune_ptr[t], p = prune_ptr[t + 1] - a, c0 = cent_ptr[t];
  const int c = cent_cnt[t];
  if (p <= 0 || c <= 0) return;                              // uniform over the workgroup
  for (int64_t base = 0; base < p; base += SZ_THREADS) {
    const int64_t i = base + tid;
    int64_t d0 = 0, d1 = 0;
    if (i < p) {
      const int d = prune_doc[a + i];
      d0 = doc_ptr[d];
      d1 = doc_ptr[d + 1];
    }
    float best = -1.f;
    int bj = 0;
    for (int j0 = 0; j0 < c; j0 += SZ_CTILE) {
      const int n = min(SZ_CTILE, c - j0);
      for (int j = tid; j < n; j += SZ_THREADS) {
        const int e = cent_doc[c0 + j0 + j];
        crow[0][j] = doc_ptr[e];
        crow[1][j] = doc_ptr[e + 1];
      }
      __syncthreads();
      if (i < p)
        for (int j = 0; j < n; ++j) {
          const float s = row_dot(doc_term, doc_w, d0, d1, doc_term, doc_w, crow[0][j], crow[1][j]);
          if (s > best) { best = s; bj = j0 + j; }         // strict: ties keep the lowest j
        }
      __syncthreads();
    }
    if (i < p) {
      assign[a + i] = bj;
      atomicAdd(&cent_size[c0 + bj], 1);
    }
  }
}

// ------------------------------------------------------------------------------------------------ build: block layout
// cursor[c0 + j] starts at centroid j's block offset; the term's kept postings (doc order) are placed 256 at a time, each
// after the earlier postings of its block: the stable counting sort by centroid.
__global__ __launch_bounds__(SZ_THREADS) void sz_fill_kernel(const int64_t* __restrict__ prune_ptr,
                                                             const int32_t* __restrict__ prune_doc,
                                                             const int32_t* __restrict__ assign,
                                                             const int64_t* __restrict__ cent_ptr,
                                                             int64_t* __restrict__ cursor,
                                                             int32_t* __restrict__ blk_doc) {
  __shared__ int sa[SZ_THREADS];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int64_t a = prune_ptr[t], p = prune_ptr[t + 1] - a, c0 = cent_ptr[t];
  for (int64_t base = 0; base < p; base += SZ_THREADS) {
    const int n = (int)min((int64_t)SZ_THREADS, p - base);
    const int my = tid < n ? assign[a + base + tid] : -1;
    sa[tid] = my;
    __syncthreads();
    int before = 0;
    bool last = true;
    for (int j = 0; j < n; ++j) {
      if (sa[j] != my) continue;
      before += j < tid;
      last = last && j <= tid;
    }
    int64_t pos = 0;
    if (tid < n) {
      pos = cursor[c0 + my] + before;
      blk_doc[pos] = prune_doc[a + base + tid];
    }
    __syncthreads();
    if (tid < n && last) cursor[c0 + my] = pos + 1;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ build: summaries
__global__ __launch_bounds__(SZ_THREADS) void sz_summary_kernel(const int64_t* __restrict__ doc_ptr,
                                                                const int32_t* __restrict__ doc_term,
                                                                const float* __restrict__ doc_w, int32_t V,
                                                                const int64_t* __restrict__ blk_ptr,
                                                                const int32_t* __restrict__ blk_doc, int64_t nblocks,
                                                                float alpha, const int64_t* __restrict__ sum_ptr,
                                                                int32_t* __restrict__ sum_cnt,
                                                                int32_t* __restrict__ sum_term,
                                                                float* __restrict__ sum_w, char* ws,
                                                                size_t slot_bytes, size_t list_off, size_t sort_off) {
  __shared__ unsigned long long sbuf[SZ_SORT_LDS];
  __shared__ int nterm, nkeep;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  char* slot = ws + (size_t)blockIdx.x * slot_bytes;
  uint32_t* M = (uint32_t*)slot;                             // [V] max weight bits of the current block, 0 = absent
  int32_t* L = (int32_t*)(slot + list_off);                  // [V] the block's distinct terms, in arrival order
  unsigned long long* G = (unsigned long long*)(slot + sort_off);
  for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
    if (tid == 0) nterm = 0;
    __syncthreads();
    const int64_t e0 = blk_ptr[b], e1 = blk_ptr[b + 1];
    for (int64_t e = e0 + wave; e < e1; e += SZ_WAVES) {     // one wave per doc, lanes over its terms
      const int d = blk_doc[e];
      const int64_t p1 = doc_ptr[d + 1];
      for (int64_t j = doc_ptr[d] + lane; j < p1; j += 64) {
        const int u = doc_term[j];
        if (atomicMax(&M[u], fbits(doc_w[j])) == 0u) L[atomicAdd(&nterm, 1)] = u;
      }
    }
    __syncthreads();
    const int n = nterm;
    const long P = pow2_at_least((long)n);
    unsigned long long* buf = P <= SZ_SORT_LDS ? sbuf : G;
    for (long i = tid; i < P; i += SZ_THREADS) {             // (m desc, u asc); the padding 0 sorts last
      unsigned long long kk = 0ull;
      if (i < n) {
        const int u = L[i];
        kk = rank_key(__hip_atomic_load(&M[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), (uint32_t)u);
      }
      buf[i] = kk;
    }
    __syncthreads();
    bitonic_desc<SZ_THREADS>(buf, P);
    if (tid == 0) {                                          // the fp32 left folds, in sorted order
      float total = 0.f;
      for (int i = 0; i < n; ++i) total = total + bitsf(rank_bits(buf[i]));
      const float goal = alpha * total;
      float acc = 0.f;
      int keep = 0;
      for (int i = 0; i < n; ++i) {
        acc = acc + bitsf(rank_bits(buf[i]));
        keep = i + 1;
        if (acc >= goal) break;
      }
      nkeep = keep;
      if (!sum_ptr) sum_cnt[b] = keep;
    }
    __syncthreads();
    const int keep = nkeep;
    if (sum_ptr) {                                           // the kept prefix, re-sorted by term ascending
      for (long i = tid; i < P; i += SZ_THREADS) {
        const unsigned long long kk = buf[i];
        buf[i] = i < keep ? ((kk & 0xFFFFFFFFull) << 32) | (kk >> 32) : 0ull;   // (~u) << 32 | m: desc = u asc
      }
      __syncthreads();
      bitonic_desc<SZ_THREADS>(buf, pow2_at_least((long)keep));
      const int64_t o = sum_ptr[b];
      for (int i = tid; i < keep; i += SZ_THREADS) {
        const unsigned long long kk = buf[i];
        sum_term[o + i] = (int32_t)(0xFFFFFFFFu - (uint32_t)(kk >> 32));
        sum_w[o + i] = bitsf((uint32_t)(kk & 0xFFFFFFFFull));
      }
    }
    for (int i = tid; i < n; i += SZ_THREADS)                // reset the touched entries for the slot's next block
      __hip_atomic_store(&M[L[i]], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ search
struct SearchSmem {
  int32_t qt[SZ_QMAX];
  float qw[SZ_QMAX];
  int32_t cut[SZ_QMAX];
  unsigned long long H[2][SZ_KMAX];              // the top k keys, descending
  unsigned long long cand[SZ_THREADS];
  float rsum[SZ_THREADS];
  int hcount, ncand, found;
};

__global__ __launch_bounds__(SZ_THREADS) void sz_search_kernel(
    const int64_t* __restrict__ q_ptr, const int32_t* __restrict__ q_term, const float* __restrict__ q_w,
    int32_t max_q_nnz, const int64_t* __restrict__ term_blk_ptr, const int64_t* __restrict__ blk_ptr,
    const int32_t* __restrict__ blk_doc, const int64_t* __restrict__ sum_ptr, const int32_t* __restrict__ sum_term,
    const float* __restrict__ sum_w, const int64_t* __restrict__ doc_ptr, const int32_t* __restrict__ doc_term,
    const float* __restrict__ doc_w, int32_t nd, int32_t V, const int32_t* __restrict__ target, int32_t k,
    int32_t top_n, float hf, int32_t* __restrict__ out_doc, float* __restrict__ out_score,
    int32_t* __restrict__ out_rank, float* __restrict__ out_tscore, int64_t* __restrict__ out_stats) {
  __shared__ SearchSmem S;
  const int tid = threadIdx.x, q = blockIdx.x;
  const int64_t qa = q_ptr[q];
  int nq = (int)(q_ptr[q + 1] - qa);
  if (nq > max_q_nnz || nq > SZ_QMAX) nq = 0;                // beyond the caller's declared cap: never past the LDS rows
  for (int i = tid; i < nq; i += SZ_THREADS) { S.qt[i] = q_term[qa + i]; S.qw[i] = q_w[qa + i]; }
  if (tid == 0) { S.hcount = 0; S.ncand = 0; S.found = 0; }
  __syncthreads();
  const int ncut = min(nq, top_n);
  for (int i = tid; i < nq; i += SZ_THREADS) {               // the cut: top_n by (weight desc, term asc)
    const float w = S.qw[i];
    int r = 0;
    for (int j = 0; j < nq; ++j) r += S.qw[j] > w || (S.qw[j] == w && j < i);   // terms ascend with the index
    if (r < ncut) S.cut[r] = i;
  }
  __syncthreads();
  const int32_t* qt = S.qt;
  const float* qw = S.qw;
  int cur = 0;
  int64_t st_total = 0, st_scored = 0, st_post = 0;
  for (int ci = 0; ci < ncut; ++ci) {
    const int t = S.qt[S.cut[ci]];
    const bool ok = (unsigned)t < (unsigned)V;
    const int64_t b0 = ok ? term_blk_ptr[t] : 0, b1 = ok ? term_blk_ptr[t + 1] : 0;
    st_total += b1 - b0;
    for (int64_t bb = b0; bb < b1; bb += SZ_THREADS) {
      const int nb = (int)min((int64_t)SZ_THREADS, b1 - bb);
      if (tid < nb) S.rsum[tid] = row_dot(qt, qw, 0, nq, sum_term, sum_w, sum_ptr[bb + tid], sum_ptr[bb + tid + 1]);
      __syncthreads();
      for (int jb = 0; jb < nb; ++jb) {
        if (S.hcount == k) {
          const float sk = bitsf(rank_bits(S.H[cur][k - 1]));
          if (hf * S.rsum[jb] < sk) continue;                // a NaN product skips nothing
        }
        const int64_t e0 = blk_ptr[bb + jb], e1 = blk_ptr[bb + jb + 1];
        ++st_scored;
        st_post += e1 - e0;
        for (int64_t e = e0; e < e1; e += SZ_THREADS) {
          const int hc0 = S.hcount;
          const unsigned long long* Hc = S.H[cur];
          if (e + tid < e1) {
            const int d = blk_doc[e + tid];
            const float s = row_dot(qt, qw, 0, nq, doc_term, doc_w, doc_ptr[d], doc_ptr[d + 1]);
            unsigned long long key = s > 0.f ? rank_key(fbits(s), (uint32_t)d) : 0ull;
            if (key && hc0 == k && key <= Hc[k - 1]) key = 0ull;
            if (key) {                                       // already in H (the same doc from an earlier block)?
              int lo = 0, hi = hc0;
              while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (Hc[mid] > key) lo = mid + 1; else hi = mid;
              }
              if (lo < hc0 && Hc[lo] == key) key = 0ull;
            }
            if (key) S.cand[atomicAdd(&S.ncand, 1)] = key;
          }
          __syncthreads();
          const int m = S.ncand;
          __syncthreads();
          if (m) {                                           // H' = top k of H + cand, every key placed by its rank
            unsigned long long* Hn = S.H[cur ^ 1];
            for (int x = tid; x < hc0; x += SZ_THREADS) {
              const unsigned long long v = Hc[x];
              int pos = x;
              for (int y = 0; y < m; ++y) pos += S.cand[y] > v;
              if (pos < k) Hn[pos] = v;
            }
            for (int y = tid; y < m; y += SZ_THREADS) {
              const unsigned long long v = S.cand[y];
              int lo = 0, hi = hc0;
              while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (Hc[mid] > v) lo = mid + 1; else hi = mid;
              }
              int pos = lo;
              for (int z = 0; z < m; ++z) pos += S.cand[z] > v;
              if (pos < k) Hn[pos] = v;
            }
          }
          if (tid == 0) {
            S.ncand = 0;
            if (m) S.hcount = min(k, hc0 + m);
          }
          __syncthreads();
          if (m) cur ^= 1;
        }
      }
      __syncthreads();                                       // rsum is rewritten by the next batch of blocks
    }
  }
  const int hc = S.hcount;
  const int tt = target ? target[q] : -1;
  for (int i = tid; i < k; i += SZ_THREADS) {
    float s = 0.f;
    int d = -1;
    if (i < hc) {
      const unsigned long long v = S.H[cur][i];
      s = bitsf(rank_bits(v));
      d = rank_id(v);
      if (d == tt) S.found = i + 1;
    }
    out_score[(int64_t)q * k + i] = s;
    out_doc[(int64_t)q * k + i] = d;
  }
  __syncthreads();
  if (tid == 0) {
    if (target) {
      out_rank[q] = S.found;
      out_tscore[q] = (unsigned)tt < (unsigned)nd
                          ? row_dot(qt, qw, 0, nq, doc_term, doc_w, doc_ptr[tt], doc_ptr[tt + 1]) : 0.f;
    }
    out_stats[(int64_t)q * 3 + 0] = st_total;
    out_stats[(int64_t)q * 3 + 1] = st_scored;
    out_stats[(int64_t)q * 3 + 2] = st_post;
  }
}

inline size_t summary_list_off(int32_t V) { return align256((size_t)V * 4); }
inline size_t summary_sort_off(int32_t V) { return 2 * align256((size_t)V * 4); }
inline size_t summary_slot_bytes(int32_t V) { return summary_sort_off(V) + align256((size_t)pow2_at_least((long)V) * 8); }

}  // namespace

extern "C" size_t snx_seismic_build_workspace_bytes(int32_t V, int64_t nblocks) {
  if (V <= 0 || nblocks <= 0) return 0;
  return (size_t)(nblocks < SZ_SLOTS ? nblocks : SZ_SLOTS) * summary_slot_bytes(V);
}

extern "C" int snx_seismic_build_clusters(const int64_t* term_ptr, const int32_t* post_doc, const float* post_w,
                                          const int64_t* doc_ptr, const int32_t* doc_term, const float* doc_w,
                                          int32_t nd, int32_t V, int32_t n_postings, const int64_t* prune_ptr,
                                          const int32_t* cent_cnt, const int64_t* cent_ptr, int64_t npruned,
                                          int64_t ncent, int32_t* prune_doc, float* prune_w, int32_t* cent_doc,
                                          int32_t* assign, int32_t* cent_size, hipStream_t st) {
  if (!term_ptr || !doc_ptr || !prune_ptr || !cent_cnt || !cent_ptr) return SNX_E_ARG;
  if (nd < 0 || V <= 0 || n_postings < 1 || npruned < 0 || ncent < 0 || ncent > npruned) return SNX_E_SHAPE;
  if (npruned == 0) return SNX_OK;
  if (!post_doc || !post_w || !doc_term || !doc_w || !prune_doc || !prune_w || !cent_doc || !assign || !cent_size)
    return SNX_E_ARG;
  const hipError_t e = hipMemsetAsync(cent_size, 0, (size_t)ncent * sizeof(int32_t), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sz_prune_kernel, dim3(V), dim3(SZ_THREADS), 0, st, term_ptr, post_doc, post_w, n_postings,
                     prune_ptr, prune_doc, prune_w);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(sz_centroid_kernel, dim3(V), dim3(SZ_THREADS), 0, st, prune_ptr, (const int32_t*)prune_doc,
                     (const float*)prune_w, cent_cnt, cent_ptr, cent_doc);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(sz_assign_kernel, dim3(V), dim3(SZ_THREADS), 0, st, prune_ptr, (const int32_t*)prune_doc,
                     cent_cnt, cent_ptr, (const int32_t*)cent_doc, doc_ptr, doc_term, doc_w, assign, cent_size);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_seismic_build_blocks(const int64_t* prune_ptr, const int32_t* prune_doc, const int32_t* assign,
                                        const int64_t* cent_ptr, int32_t V, int64_t npruned, int64_t* cursor,
                                        int32_t* blk_doc, hipStream_t st) {
  if (!prune_ptr || !cent_ptr) return SNX_E_ARG;
  if (V <= 0 || npruned < 0) return SNX_E_SHAPE;
  if (npruned == 0) return SNX_OK;
  if (!prune_doc || !assign || !cursor || !blk_doc) return SNX_E_ARG;
  hipLaunchKernelGGL(sz_fill_kernel, dim3(V), dim3(SZ_THREADS), 0, st, prune_ptr, prune_doc, assign, cent_ptr, cursor,
                     blk_doc);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_seismic_build_summaries(const int64_t* doc_ptr, const int32_t* doc_term, const float* doc_w,
                                           int32_t nd, int32_t V, const int64_t* blk_ptr, const int32_t* blk_doc,
                                           int64_t nblocks, float alpha, const int64_t* sum_ptr, int32_t* sum_cnt,
                                           int32_t* sum_term, float* sum_w, void* workspace, size_t ws_bytes,
                                           hipStream_t st) {
  if (!doc_ptr || !blk_ptr) return SNX_E_ARG;
  if (nd < 0 || V <= 0 || nblocks < 0 || !(alpha > 0.f) || !(alpha <= 1.f)) return SNX_E_SHAPE;
  if (nblocks == 0) return SNX_OK;
  if (!doc_term || !doc_w || !blk_doc) return SNX_E_ARG;
  if (sum_ptr ? (!sum_term || !sum_w) : !sum_cnt) return SNX_E_ARG;
  const size_t need = snx_seismic_build_workspace_bytes(V, nblocks);
  if (!workspace || ws_bytes < need) return SNX_E_ARG;
  const int grid = (int)(nblocks < SZ_SLOTS ? nblocks : SZ_SLOTS);
  const size_t slot = summary_slot_bytes(V);
  for (int g = 0; g < grid; ++g) {                           // the max tables start at 0 (each block resets its entries)
    const hipError_t e = hipMemsetAsync((char*)workspace + (size_t)g * slot, 0, (size_t)V * 4, st);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(sz_summary_kernel, dim3(grid), dim3(SZ_THREADS), 0, st, doc_ptr, doc_term, doc_w, V, blk_ptr,
                     blk_doc, nblocks, alpha, sum_ptr, sum_cnt, sum_term, sum_w, (char*)workspace, slot,
                     summary_list_off(V), summary_sort_off(V));
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_seismic_search(const int64_t* q_ptr, const int32_t* q_term, const float* q_w, int32_t nq,
                                  int32_t max_q_nnz, const int64_t* term_blk_ptr, const int64_t* blk_ptr,
                                  const int32_t* blk_doc, const int64_t* sum_ptr, const int32_t* sum_term,
                                  const float* sum_w, const int64_t* doc_ptr, const int32_t* doc_term,
                                  const float* doc_w, int32_t nd, int32_t V, const int32_t* target, int32_t k,
                                  int32_t top_n, float heap_factor, int32_t* out_doc, float* out_score,
                                  int32_t* out_rank, float* out_tscore, int64_t* out_stats, hipStream_t st) {
  if (!q_ptr || !term_blk_ptr || !blk_ptr || !sum_ptr || !doc_ptr || !out_doc || !out_score || !out_stats)
    return SNX_E_ARG;
  if (target && (!out_rank || !out_tscore)) return SNX_E_ARG;
  if (nq < 0 || nd < 0 || V <= 0 || k < 1 || k > SZ_KMAX || top_n < 1 || max_q_nnz < 0 || max_q_nnz > SZ_QMAX ||
      !(heap_factor > 0.f))
    return SNX_E_SHAPE;
  if (nq == 0) return SNX_OK;
  hipLaunchKernelGGL(sz_search_kernel, dim3(nq), dim3(SZ_THREADS), 0, st, q_ptr, q_term, q_w, max_q_nnz, term_blk_ptr,
                     blk_ptr, blk_doc, sum_ptr, sum_term, sum_w, doc_ptr, doc_term, doc_w, nd, V, target, k, top_n,
                     heap_factor, out_doc, out_score, out_rank, out_tscore, out_stats);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}
