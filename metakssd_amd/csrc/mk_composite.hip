/*
 * mk_composite.hip -- `composite -r <markerdb> -q <sketch_dir>` with the marker database resident on the device.
 *
 * get_species_abundance() (command_composite.c:446-640) reads, for every query sample and component, the whole reference
 * component again and walks all of its ids.  Here the join is turned round: the database is inverted once (k-mer id -> the
 * reference sketches that hold it, as combco2mco() does, co2mco.c:37-59) and stays in HBM; a sample then looks up only its own ids.
 *
 *   load, per component
 *     mkc_gid_kernel          position in combco.N -> reference sketch number (binary search in combco.index.N)
 *     mk_radix_sort_pairs_u32 (id, sketch) by id, STABLE; duplicates stay (an id twice in one sketch is two entries of its row)
 *     mkc_count/scan/emit<RowF>   ordered compaction of the row heads: distinct ids + row starts
 *     mkc_bucket_kernel       bucket table on the high bits of the id in front of the binary search
 *   query, per component of a batch of samples
 *     mkc_lookup_kernel       one thread per query position: its row (or none); a position with a row enters an open-addressing
 *                             table keyed on (sample, id) that keeps the MINIMUM position -- the reference's dictionary finds the
 *                             first occurrence of an id in a sample (command_composite.c:538-546, :551-554)
 *     mkc_winner_kernel       a position that is not the minimum of its key loses its row; the others add their row's length to
 *                             the sample's hit count
 *   a sample that arrives as a device key list (mk_composite_query_sample_keys)
 *     mkc_part_count_kernel   per-block LDS histogram of key % comp_num -> the sample's size in every component
 *     mkc_part_scatter_kernel (id, count) of every key appended to its component's query arrays; order inside a slice is free
 *     mkc_lookup_kernel<true>, mkc_winner_kernel<true>  at the finish of such a batch: the keys of a sample are distinct, so no id
 *                             repeats in a sample, the (sample, id) table is not needed and every position with a row counts
 *   finish, per sub-range of whole samples (hits <= the hit buffer, samples * ref_num <= 2^32 - 1)
 *     mkc_count/scan/emit<HitF>   per component: one hit (segment = local sample * ref_num + sketch, count) per row entry, all
 *                             components into one buffer (the reference accumulates over components before it sorts, :496-574)
 *     mk_radix_sort_pairs_u32 by count (16 bits: the two upper passes find one digit and are skipped), then stable by segment
 *     mkc_count/scan/emit<HeadF>, <BigF>   segment starts; the segments with kmer_num >= 6 (MIN_KM_S, :600)
 *     mkc_stats_kernel        a wave per segment: the integers of :599-613
 *   The rows of a sample are put into print order (kmer_num descending, reference number ascending among equals: what glibc's
 *   merge-sort qsort gives the reference, :584) on the host; the float divisions of :618/:624 stay with the caller.
 *
 * Everything is integer work without contraction: HBM- and latency-bound, MFMA does not apply.  No CPU path.
 */
#pragma clang fp contract(off) /* the two double products of :607/:610 are the reference's: nothing fuses into them */
#include <hip/hip_runtime.h>
#include "mk_poison.hip.h"

namespace { /* mk_mco.hip and mk_abv.hip hold the sort's kernels too: this file's copies stay local */
#include "mk_sort.hip.h"
}

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "metakssd_hip.h"

#define MKC_BLOCK 256u
#define MKC_NONE 0xFFFFFFFFu
#define MKC_EMPTY 0xFFFFFFFFFFFFFFFFull
#define MKC_MIN_KM 6u                  /* MIN_KM_S */
#define MKC_BUCKET_BITS 20u            /* at most 2^20 buckets (4 MiB) per component */
#define MKC_DEFAULT_MAX_HITS (1ull << 26) /* 64 M hits: four 256 MiB arrays */
#define MKC_PART_MAX 16u               /* components a device key list is split into (mk_composite_query_sample_keys) */
enum { MKC_BATCH_NONE = 0, MKC_BATCH_HOST, MKC_BATCH_DEVICE };

struct mkc_comp {
  bool loaded = false;
  uint64_t n = 0, nrows = 0;
  uint32_t *d_row_ids = nullptr;   /* [nrows] ascending distinct ids */
  uint32_t *d_row_start = nullptr; /* [nrows + 1] */
  uint32_t *d_refs = nullptr;      /* [n] reference sketch numbers, row after row, a row in sketch order */
  uint32_t *d_bucket = nullptr;    /* [nbuckets + 1] first row whose id >> shift is >= the bucket */
  uint32_t shift = 0, nbuckets = 0;
  /* the current batch */
  bool have = false;
  uint64_t nq = 0;
  uint32_t *d_qids = nullptr, *d_rowidx = nullptr;
  uint16_t *d_qcnt = nullptr;
  unsigned long long *d_qindex = nullptr;
  uint64_t q_cap = 0, qcnt_cap = 0, rowidx_cap = 0, qindex_cap = 0;
  std::vector<uint64_t> qindex;
};

struct mk_composite {
  int device = 0, num_cu = 256;
  hipStream_t stream = nullptr;
  uint32_t ref_num = 0, comp_num = 0, nsamples = 0;
  bool load_begun = false, querying = false;
  int batch_kind = MKC_BATCH_NONE; /* who feeds the current batch: mk_composite_query_component or mk_composite_query_sample_keys */
  uint32_t next_k = 0;             /* device-fed batch: the sample that comes next */
  unsigned long long *d_part = nullptr, *h_part = nullptr; /* [2 * MKC_PART_MAX] a key list's component totals and scatter cursors; [MKC_PART_MAX] pinned */
  uint64_t max_hits = MKC_DEFAULT_MAX_HITS;
  std::vector<mkc_comp> comp;
  /* sort scratch, shared by load and finish */
  uint32_t *d_key[2] = {nullptr, nullptr}, *d_val[2] = {nullptr, nullptr};
  uint64_t pair_cap = 0;
  void *d_tmp = nullptr;
  uint32_t *h_sort_flag = nullptr;
  unsigned long long *d_index = nullptr;
  uint64_t index_cap = 0;
  unsigned long long *d_blk = nullptr;
  uint64_t blk_cap = 0;
  unsigned long long *d_base = nullptr; /* [comp_num + 2] running totals of a compaction chain */
  uint64_t base_cap = 0;
  unsigned long long *h_word = nullptr; /* pinned, 2 words */
  /* (sample, id) -> first position */
  unsigned long long *d_tkey = nullptr;
  uint32_t *d_tpos = nullptr;
  uint64_t tkey_cap = 0, tpos_cap = 0;
  unsigned long long *d_sample_hits = nullptr, *h_sample_hits = nullptr;
  uint64_t sample_cap = 0, h_sample_cap = 0;
  uint32_t *d_starts = nullptr, *d_big = nullptr;
  uint64_t starts_cap = 0, big_cap = 0;
  mk_composite_row *d_rows = nullptr, *h_rows = nullptr;
  uint64_t rows_cap = 0, h_rows_cap = 0;
  std::vector<mk_composite_row> rows; /* the last finish's result */
  std::vector<uint32_t> row_sample;
  hipEvent_t ev[2] = {nullptr, nullptr};
  double load_ms = 0.0, query_ms = 0.0;
  uint64_t hits = 0, ranges = 0;
  char err[256] = {0};
};

static thread_local char mkc_create_err[256];

static int mkc_fail(mk_composite *h, int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(h ? h->err : mkc_create_err, 256, fmt, ap);
  va_end(ap);
  return code;
}

#define MKC_HIP(h, call)                                                                          \
  do {                                                                                            \
    hipError_t _r = (call);                                                                       \
    if (_r != hipSuccess) return mkc_fail(h, MK_ERR_HIP, "%s: %s", #call, hipGetErrorString(_r)); \
  } while (0)

template <class T>
static int mkc_grow(mk_composite *h, T **p, uint64_t *cap, uint64_t need, bool slack = true) {
  if (need <= *cap && *p) return MK_OK;
  (void)hipFree(*p);
  *p = nullptr; *cap = 0;
  const uint64_t c = slack ? need + need / 8 + 1024 : (need ? need : 1);
  hipError_t r = mk_dev_alloc((void **)p, c * sizeof(T));
  if (r != hipSuccess) { *p = nullptr; return mkc_fail(h, MK_ERR_NOMEM, "device allocation of %llu bytes: %s", (unsigned long long)(c * sizeof(T)), hipGetErrorString(r)); }
  *cap = c;
  return MK_OK;
}

/* ---- kernels ------------------------------------------------------------------------------------------ */

/* number of entries of a[lo..hi) that are <= x */
template <class T, class X>
__device__ __forceinline__ uint64_t mkc_upper(const T *a, uint64_t lo, uint64_t hi, X x) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if ((X)a[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
/* number of entries of a[lo..hi) that are < x */
template <class T, class X>
__device__ __forceinline__ uint64_t mkc_lower(const T *a, uint64_t lo, uint64_t hi, X x) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if ((X)a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(MKC_BLOCK) mkc_gid_kernel(const unsigned long long *index, uint32_t ref_num, uint64_t n, uint32_t *gid) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    gid[i] = (uint32_t)(mkc_upper(index, 0, (uint64_t)ref_num + 1, (unsigned long long)i) - 1);
}

/* exclusive prefix of v over the workgroup's MKC_BLOCK threads (every thread of the block calls it); *total = the block's sum */
__device__ __forceinline__ unsigned long long mkc_block_excl(unsigned long long v, unsigned long long *total) {
  __shared__ unsigned long long ws[MKC_BLOCK / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long u = __shfl_up(incl, o);
    if ((int)lane >= o) incl += u;
  }
  if (lane == 63u) ws[wave] = incl;
  __syncthreads();
  unsigned long long woff = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < MKC_BLOCK / 64; w++) { if (w < wave) woff += ws[w]; all += ws[w]; }
  __syncthreads(); /* ws may be written again by the next call */
  *total = all;
  return woff + incl - v;
}

/* The ordered-compaction pattern: a functor says how many outputs position i has (count) and writes them at their place (emit).
 *   mkc_count_kernel  per block of MKC_BLOCK positions: the block's number of outputs
 *   mkc_scan_kernel   one workgroup: exclusive prefix over the blocks, started at *base_in; *total_out = *base_in + everything
 *   mkc_emit_kernel   the counts again, the place inside the block by a block scan, emit */
template <class F>
__global__ void __launch_bounds__(MKC_BLOCK) mkc_count_kernel(F f, uint64_t n, unsigned long long *blk) {
  const uint64_t i = (uint64_t)blockIdx.x * MKC_BLOCK + threadIdx.x;
  unsigned long long tot;
  (void)mkc_block_excl(i < n ? f.count(i) : 0ull, &tot);
  if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(1024) mkc_scan_kernel(unsigned long long *blk, uint64_t nblk, const unsigned long long *base_in,
                                                       unsigned long long *total_out) {
  __shared__ unsigned long long part[1024];
  const uint32_t t = threadIdx.x;
  const uint64_t per = (nblk + 1023u) / 1024u, lo = (uint64_t)t * per < nblk ? (uint64_t)t * per : nblk, hi = lo + per < nblk ? lo + per : nblk;
  unsigned long long sum = 0;
  for (uint64_t k = lo; k < hi; k++) sum += blk[k];
  part[t] = sum;
  __syncthreads();
  for (uint32_t o = 1; o < 1024u; o <<= 1) {
    const unsigned long long v = t >= o ? part[t - o] : 0ull;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  const unsigned long long base = base_in ? *base_in : 0ull;
  unsigned long long run = base + part[t] - sum;
  for (uint64_t k = lo; k < hi; k++) { const unsigned long long c = blk[k]; blk[k] = run; run += c; }
  if (t == 1023u) *total_out = base + part[t];
}

template <class F>
__global__ void __launch_bounds__(MKC_BLOCK) mkc_emit_kernel(F f, uint64_t n, const unsigned long long *blk) {
  const uint64_t i = (uint64_t)blockIdx.x * MKC_BLOCK + threadIdx.x;
  const unsigned long long c = i < n ? f.count(i) : 0ull;
  unsigned long long tot;
  const unsigned long long e = mkc_block_excl(c, &tot);
  if (c) f.emit(i, blk[blockIdx.x] + e);
}

/* load: the heads of the sorted ids -> the row table */
struct mkc_row_f {
  const uint32_t *key;
  uint32_t *row_ids, *row_start;
  uint64_t cap;
  __device__ unsigned long long count(uint64_t i) const { return i == 0 || key[i] != key[i - 1] ? 1ull : 0ull; }
  __device__ void emit(uint64_t i, unsigned long long o) const {
    if (o < cap) { row_ids[o] = key[i]; row_start[o] = (uint32_t)i; }
  }
};

__global__ void mkc_set_u32_kernel(uint32_t *p, uint32_t v) { *p = v; }

/* bucket[b] = first row whose id is >= b << shift, b = 0..nbuckets (bucket[nbuckets] = nrows) */
__global__ void __launch_bounds__(MKC_BLOCK) mkc_bucket_kernel(const uint32_t *row_ids, uint64_t nrows, uint32_t shift, uint32_t nbuckets, uint32_t *bucket) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b > nbuckets) return;
  bucket[b] = b == nbuckets ? (uint32_t)nrows : (uint32_t)mkc_lower(row_ids, 0, nrows, (uint64_t)(b << shift));
}

__device__ __forceinline__ uint64_t mkc_mix(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}

/* ---- a sample as a device key list -> the per-component query arrays ----
 * Two passes over the list.  The first counts: a histogram over the components per block in LDS, one global add per block and
 * component.  The host then sizes the query arrays from the totals.  The second counts again, reserves the block's stretch of
 * every component with one global add each, and hands out the places inside the stretch by LDS adds: any order will do, the ids of a
 * sample's slice are distinct and nothing downstream reads their order (the hits are sorted by count and segment). */
struct mkc_part_dst {
  uint32_t *qids[MKC_PART_MAX];
  uint16_t *qcnt[MKC_PART_MAX];
  unsigned long long base[MKC_PART_MAX], cap[MKC_PART_MAX]; /* where the sample's slice begins; entries the arrays hold */
};

__global__ void __launch_bounds__(MKC_BLOCK) mkc_part_count_kernel(const unsigned long long *keys, uint64_t n, uint32_t comp_num, unsigned long long *totals) {
  __shared__ uint32_t hist[MKC_PART_MAX];
  if (threadIdx.x < MKC_PART_MAX) hist[threadIdx.x] = 0u;
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    atomicAdd(&hist[(uint32_t)(keys[i] % comp_num)], 1u);
  __syncthreads();
  if (threadIdx.x < comp_num && hist[threadIdx.x]) atomicAdd(&totals[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}

__global__ void __launch_bounds__(MKC_BLOCK) mkc_part_scatter_kernel(const unsigned long long *keys, const uint32_t *counts, uint64_t n, uint32_t comp_num,
                                                                    uint32_t comp_code_bits, unsigned long long *cursor, mkc_part_dst dst) {
  __shared__ uint32_t hist[MKC_PART_MAX];
  __shared__ unsigned long long start[MKC_PART_MAX];
  if (threadIdx.x < MKC_PART_MAX) hist[threadIdx.x] = 0u;
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    atomicAdd(&hist[(uint32_t)(keys[i] % comp_num)], 1u);
  __syncthreads();
  if (threadIdx.x < comp_num) {
    const uint32_t c = threadIdx.x;
    start[c] = dst.base[c] + (hist[c] ? atomicAdd(&cursor[c], (unsigned long long)hist[c]) : 0ull);
    hist[c] = 0u;
  }
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long key = keys[i];
    const uint32_t c = (uint32_t)(key % comp_num);
    const unsigned long long p = start[c] + atomicAdd(&hist[c], 1u);
    if (p < dst.cap[c]) { /* (the first pass counted them: always) */
      const uint32_t v = counts[i];
      dst.qids[c][p] = (uint32_t)(key >> comp_code_bits);
      dst.qcnt[c][p] = (uint16_t)(v > 65535u ? 65535u : v);
    }
  }
}

/* query position -> its row; positions with a row enter the (sample, id) table, which keeps the smallest position.  DISTINCT: the
 * batch came as key lists, no id repeats in a sample: no table (tkey, tpos are not read) */
template <bool DISTINCT>
__global__ void __launch_bounds__(MKC_BLOCK) mkc_lookup_kernel(const uint32_t *qids, uint64_t nq, const unsigned long long *qindex, uint32_t nsamples,
                                                              const uint32_t *row_ids, const uint32_t *bucket, uint32_t shift, uint32_t nbuckets,
                                                              unsigned long long *tkey, uint32_t *tpos, uint64_t tmask, uint32_t *rowidx) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t id = qids[i];
    const uint64_t b = (uint64_t)id >> shift;
    uint32_t row = MKC_NONE;
    if (b < nbuckets) {
      const uint64_t lo = bucket[b], hi = bucket[b + 1];
      const uint64_t r = mkc_lower(row_ids, lo, hi, id);
      if (r < hi && row_ids[r] == id) row = (uint32_t)r;
    }
    rowidx[i] = row;
    if (DISTINCT || row == MKC_NONE) continue;
    const uint64_t s = mkc_upper(qindex, 0, (uint64_t)nsamples + 1, (unsigned long long)i) - 1;
    const unsigned long long k = ((unsigned long long)s << 32) | id;
    for (uint64_t slot = mkc_mix(k) & tmask;; slot = (slot + 1) & tmask) { /* at most half of the slots are ever taken */
      const unsigned long long was = atomicCAS(&tkey[slot], MKC_EMPTY, k);
      if (was == MKC_EMPTY || was == k) { atomicMin(&tpos[slot], (uint32_t)i); break; }
    }
  }
}

/* DISTINCT: every position with a row is the only one of its (sample, id) and adds its row's length */
template <bool DISTINCT>
__global__ void __launch_bounds__(MKC_BLOCK) mkc_winner_kernel(const uint32_t *qids, uint64_t nq, const unsigned long long *qindex, uint32_t nsamples,
                                                              const uint32_t *row_start, const unsigned long long *tkey, const uint32_t *tpos,
                                                              uint64_t tmask, uint32_t *rowidx, unsigned long long *sample_hits) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t row = rowidx[i];
    if (row == MKC_NONE) continue;
    const uint64_t s = mkc_upper(qindex, 0, (uint64_t)nsamples + 1, (unsigned long long)i) - 1;
    if (!DISTINCT) {
      const unsigned long long k = ((unsigned long long)s << 32) | qids[i];
      uint64_t slot = mkc_mix(k) & tmask;
      while (tkey[slot] != k) slot = (slot + 1) & tmask; /* it is there: mkc_lookup_kernel put it in */
      if (tpos[slot] != (uint32_t)i) { rowidx[i] = MKC_NONE; continue; } /* a repeat of an id in its sample: the first occurrence counts */
    }
    atomicAdd(&sample_hits[s], (unsigned long long)(row_start[row + 1] - row_start[row]));
  }
}

/* finish: positions [p0, p0 + n) of a component -> hits */
struct mkc_hit_f {
  const uint32_t *rowidx, *row_start, *refs;
  const uint16_t *qcnt;
  const unsigned long long *qindex;
  uint32_t nsamples, s0, ref_num;
  uint64_t p0, cap;
  uint32_t *ocnt, *oseg;
  __device__ unsigned long long count(uint64_t i) const {
    const uint32_t r = rowidx[p0 + i];
    return r == MKC_NONE ? 0ull : (unsigned long long)(row_start[r + 1] - row_start[r]);
  }
  __device__ void emit(uint64_t i, unsigned long long o) const {
    const uint64_t p = p0 + i;
    const uint32_t r = rowidx[p];
    const uint32_t s = (uint32_t)(mkc_upper(qindex, 0, (uint64_t)nsamples + 1, (unsigned long long)p) - 1) - s0;
    const uint32_t c = qcnt[p], base = s * ref_num;
    const uint32_t a = row_start[r], b = row_start[r + 1];
    for (uint32_t k = a; k < b; k++, o++)
      if (o < cap) { ocnt[o] = c; oseg[o] = base + refs[k]; }
  }
};

struct mkc_head_f {
  const uint32_t *seg;
  uint32_t *starts;
  uint64_t cap;
  __device__ unsigned long long count(uint64_t i) const { return i == 0 || seg[i] != seg[i - 1] ? 1ull : 0ull; }
  __device__ void emit(uint64_t i, unsigned long long o) const { if (o < cap) starts[o] = (uint32_t)i; }
};

struct mkc_big_f {
  const uint32_t *starts;
  uint64_t nseg, nhits, cap;
  uint32_t *big;
  __device__ unsigned long long count(uint64_t j) const {
    const uint64_t e = j + 1 < nseg ? starts[j + 1] : nhits;
    return e - starts[j] >= MKC_MIN_KM ? 1ull : 0ull;
  }
  __device__ void emit(uint64_t j, unsigned long long o) const { if (o < cap) big[o] = (uint32_t)j; }
};

/* command_composite.c:599-613 for one segment per wave; v = the segment's counts, ascending (v[n - 1] is the reference's [n]) */
__global__ void __launch_bounds__(MKC_BLOCK) mkc_stats_kernel(const uint32_t *seg, const uint32_t *cnt, const uint32_t *starts, uint64_t nseg,
                                                             uint64_t nhits, const uint32_t *big, uint64_t nbig, mk_composite_row *rows) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t w = ((uint64_t)blockIdx.x * MKC_BLOCK + threadIdx.x) >> 6;
  if (w >= nbig) return; /* wave-uniform */
  const uint64_t j = big[w];
  const uint64_t a = starts[j], e = j + 1 < nseg ? starts[j + 1] : nhits;
  const uint32_t *v = cnt + a;
  const uint32_t kn = (uint32_t)(e - a);
  uint32_t sum = 0; /* two's complement, as the reference's int */
  for (uint32_t n = lane; n < kn; n += 64u) sum += v[n];
  const int pct_idx = (int)((double)(int)kn * 0.98);                /* :607 */
  const int last = (int)__builtin_floor((double)(int)kn * 0.99);    /* :610: the largest n with n <= kmer_num * 0.99 */
  uint32_t lastsum = 0;
  for (int n = pct_idx + (int)lane; n <= last; n += 64) lastsum += v[n - 1];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { sum += __shfl_down(sum, off, 64); lastsum += __shfl_down(lastsum, off, 64); }
  if (lane == 0) {
    mk_composite_row r;
    r.ref = seg[a]; /* the segment number: the host splits it into sample and reference */
    r.kmer_num = (int32_t)kn;
    r.sum = (int32_t)sum;
    r.lastsum = (int32_t)lastsum;
    r.lastn = last >= pct_idx ? last - pct_idx + 1 : 0;
    r.median = (int32_t)v[kn / 2u - 1u];
    r.top = (int32_t)v[kn - 1u];
    rows[w] = r;
  }
}

/* ---- host side ---------------------------------------------------------------------------------------- */

static void mkc_free_comp(mkc_comp &c) {
  (void)hipFree(c.d_row_ids); (void)hipFree(c.d_row_start); (void)hipFree(c.d_refs); (void)hipFree(c.d_bucket);
  (void)hipFree(c.d_qids); (void)hipFree(c.d_rowidx); (void)hipFree(c.d_qcnt); (void)hipFree(c.d_qindex);
  c = mkc_comp();
}

extern "C" int mk_composite_create(int device, mk_composite **out) {
  if (!out) return MK_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return mkc_fail(nullptr, MK_ERR_NO_DEVICE, "no HIP device: mk_composite has no CPU path");
  if (device < 0 || device >= ndev) return mkc_fail(nullptr, MK_ERR_NO_DEVICE, "device %d out of range (0..%d)", device, ndev - 1);
  mk_composite *h = new (std::nothrow) mk_composite();
  if (!h) return MK_ERR_NOMEM;
  h->device = device;
  hipDeviceProp_t prop;
  if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) {
    delete h;
    return mkc_fail(nullptr, MK_ERR_NO_DEVICE, "hipSetDevice(%d) failed", device);
  }
  h->num_cu = prop.multiProcessorCount;
  hipError_t r = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (r == hipSuccess) r = mk_dev_alloc(&h->d_tmp, (size_t)256 * MK_RS_MAXB * 4 + 256 * 8 + 64);
  if (r == hipSuccess) r = mk_pin_alloc((void **)&h->h_sort_flag, 4 * sizeof(uint32_t), hipHostMallocDefault);
  if (r == hipSuccess) r = mk_pin_alloc((void **)&h->h_word, 16, hipHostMallocDefault);
  if (r == hipSuccess) r = mk_pin_alloc((void **)&h->h_part, MKC_PART_MAX * sizeof(unsigned long long), hipHostMallocDefault);
  if (r == hipSuccess) r = mk_dev_alloc((void **)&h->d_part, 2 * MKC_PART_MAX * sizeof(unsigned long long));
  if (r == hipSuccess) r = hipEventCreate(&h->ev[0]);
  if (r == hipSuccess) r = hipEventCreate(&h->ev[1]);
  if (r != hipSuccess) {
    mkc_fail(nullptr, MK_ERR_NOMEM, "mk_composite allocation: %s", hipGetErrorString(r));
    mk_composite_destroy(h);
    return MK_ERR_NOMEM;
  }
  *out = h;
  return MK_OK;
}

extern "C" int mk_composite_destroy(mk_composite *h) {
  if (!h) return MK_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (auto &c : h->comp) mkc_free_comp(c);
  for (int b = 0; b < 2; b++) { (void)hipFree(h->d_key[b]); (void)hipFree(h->d_val[b]); if (h->ev[b]) (void)hipEventDestroy(h->ev[b]); }
  (void)hipFree(h->d_tmp); (void)hipFree(h->d_index); (void)hipFree(h->d_blk); (void)hipFree(h->d_base); (void)hipFree(h->d_tkey);
  (void)hipFree(h->d_tpos); (void)hipFree(h->d_sample_hits); (void)hipFree(h->d_starts); (void)hipFree(h->d_big); (void)hipFree(h->d_rows);
  if (h->h_sort_flag) (void)hipHostFree(h->h_sort_flag);
  if (h->h_word) (void)hipHostFree(h->h_word);
  if (h->h_part) (void)hipHostFree(h->h_part);
  (void)hipFree(h->d_part);
  if (h->h_sample_hits) (void)hipHostFree(h->h_sample_hits);
  if (h->h_rows) (void)hipHostFree(h->h_rows);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return MK_OK;
}

extern "C" const char *mk_composite_last_error(const mk_composite *h) { return h ? h->err : mkc_create_err; }

extern "C" int mk_composite_set_option(mk_composite *h, int option, int64_t value) {
  if (!h) return MK_ERR_ARG;
  switch (option) {
    case MK_COMPOSITE_OPT_MAX_HITS:
      if (value < 1 || (uint64_t)value >= (1ull << 32)) return mkc_fail(h, MK_ERR_ARG, "MK_COMPOSITE_OPT_MAX_HITS: 1 .. 2^32 - 1");
      h->max_hits = (uint64_t)value;
      return MK_OK;
    default: return mkc_fail(h, MK_ERR_ARG, "unknown mk_composite option %d", option);
  }
}

static unsigned mkc_blocks(const mk_composite *h, uint64_t n) {
  uint64_t b = (n + MKC_BLOCK - 1) / MKC_BLOCK;
  const uint64_t cap = (uint64_t)h->num_cu * 32u;
  if (b > cap) b = cap;
  return b ? (unsigned)b : 1u;
}

static int mkc_time_begin(mk_composite *h) {
  MKC_HIP(h, hipEventRecord(h->ev[0], h->stream));
  return MK_OK;
}
static int mkc_time_end(mk_composite *h, double *acc) {
  float f = 0.f;
  MKC_HIP(h, hipEventRecord(h->ev[1], h->stream));
  MKC_HIP(h, hipEventSynchronize(h->ev[1]));
  MKC_HIP(h, hipEventElapsedTime(&f, h->ev[0], h->ev[1]));
  *acc += (double)f;
  return MK_OK;
}

/* count + scan + (total to the host) of a compaction over n positions; the caller allocates the output and calls mkc_emit */
template <class F>
static int mkc_compact_count(mk_composite *h, const F &f, uint64_t n, const unsigned long long *base_in, unsigned long long *total_out) {
  const uint64_t nblk = (n + MKC_BLOCK - 1) / MKC_BLOCK;
  int rc = mkc_grow(h, &h->d_blk, &h->blk_cap, nblk);
  if (rc) return rc;
  hipLaunchKernelGGL(mkc_count_kernel<F>, dim3((unsigned)nblk), dim3(MKC_BLOCK), 0, h->stream, f, n, h->d_blk);
  hipLaunchKernelGGL(mkc_scan_kernel, dim3(1), dim3(1024), 0, h->stream, h->d_blk, nblk, base_in, total_out);
  MKC_HIP(h, hipGetLastError());
  return MK_OK;
}
template <class F>
static int mkc_compact_emit(mk_composite *h, const F &f, uint64_t n) {
  const uint64_t nblk = (n + MKC_BLOCK - 1) / MKC_BLOCK;
  hipLaunchKernelGGL(mkc_emit_kernel<F>, dim3((unsigned)nblk), dim3(MKC_BLOCK), 0, h->stream, f, n, (const unsigned long long *)h->d_blk);
  MKC_HIP(h, hipGetLastError());
  return MK_OK;
}
static int mkc_fetch_word(mk_composite *h, const unsigned long long *d, uint64_t *out) {
  MKC_HIP(h, hipMemcpyAsync(h->h_word, d, 8, hipMemcpyDeviceToHost, h->stream));
  MKC_HIP(h, hipStreamSynchronize(h->stream));
  *out = h->h_word[0];
  return MK_OK;
}

static int mkc_grow_pairs(mk_composite *h, uint64_t n) {
  if (n <= h->pair_cap && h->d_key[0]) return MK_OK;
  uint64_t cap = 0;
  for (int b = 0; b < 2; b++) {
    int rc;
    cap = h->pair_cap;
    if ((rc = mkc_grow(h, &h->d_key[b], &cap, n))) { h->pair_cap = 0; return rc; }
    cap = h->pair_cap;
    if ((rc = mkc_grow(h, &h->d_val[b], &cap, n))) { h->pair_cap = 0; return rc; }
  }
  h->pair_cap = cap;
  return MK_OK;
}

static hipError_t mkc_sort(mk_composite *h, uint32_t *key[2], uint32_t *val[2], uint64_t n, int *where) {
  uint32_t *hist = (uint32_t *)h->d_tmp;
  unsigned long long *tot = (unsigned long long *)((uint8_t *)h->d_tmp + (size_t)256 * MK_RS_MAXB * 4);
  uint32_t *flag = (uint32_t *)((uint8_t *)h->d_tmp + (size_t)256 * MK_RS_MAXB * 4 + 256 * 8);
  return mk_radix_sort_pairs_u32(key, val, n, h->num_cu, hist, tot, flag, h->h_sort_flag, h->stream, where);
}

extern "C" int mk_composite_load_begin(mk_composite *h, uint32_t ref_num, uint32_t comp_num) {
  if (!h) return MK_ERR_ARG;
  MKC_HIP(h, hipSetDevice(h->device));
  MKC_HIP(h, hipStreamSynchronize(h->stream));
  for (auto &c : h->comp) mkc_free_comp(c);
  h->comp.clear();
  h->load_begun = false; h->querying = false;
  try { h->comp.resize(comp_num); } catch (...) { return mkc_fail(h, MK_ERR_NOMEM, "mk_composite_load_begin: %u components", comp_num); }
  int rc = mkc_grow(h, &h->d_base, &h->base_cap, (uint64_t)comp_num + 2);
  if (rc) return rc;
  h->ref_num = ref_num; h->comp_num = comp_num;
  h->load_ms = 0.0; h->query_ms = 0.0;
  h->load_begun = true;
  return MK_OK;
}

extern "C" int mk_composite_load_component(mk_composite *h, uint32_t ci, const uint32_t *ref_ids, const uint64_t *ref_index) {
  if (!h || !ref_index) return MK_ERR_ARG;
  if (!h->load_begun) return mkc_fail(h, MK_ERR_STATE, "mk_composite_load_component before mk_composite_load_begin");
  if (h->querying) return mkc_fail(h, MK_ERR_STATE, "mk_composite_load_component inside a query batch");
  if (ci >= h->comp_num) return mkc_fail(h, MK_ERR_ARG, "component %u of %u", ci, h->comp_num);
  const uint32_t R = h->ref_num;
  const uint64_t n = ref_index[R];
  if (n && !ref_ids) return MK_ERR_ARG;
  /* the sort keeps its per-(digit, workgroup) prefixes in 32 bits (mk_sort.hip.h): as for mk_mco_build */
  if (n >= (1ull << 32)) return mkc_fail(h, MK_ERR_ARG, "mk_composite_load_component: a component of %llu ids (fewer than 2^32 are supported)", (unsigned long long)n);
  if (ref_index[0] != 0) return mkc_fail(h, MK_ERR_ARG, "combco.index does not start at 0");
  for (uint32_t j = 0; j < R; j++)
    if (ref_index[j] > ref_index[j + 1]) return mkc_fail(h, MK_ERR_ARG, "combco.index not ascending at sketch %u", j);
  MKC_HIP(h, hipSetDevice(h->device));
  mkc_comp &c = h->comp[ci];
  mkc_free_comp(c);
  c.n = n;
  int rc;
  if (n) {
    uint64_t cap = 0;
    if ((rc = mkc_grow_pairs(h, n))) return rc;
    if ((rc = mkc_grow(h, &h->d_index, &h->index_cap, (uint64_t)R + 1))) return rc;
    MKC_HIP(h, hipMemcpyAsync(h->d_index, ref_index, ((size_t)R + 1) * 8, hipMemcpyHostToDevice, h->stream));
    MKC_HIP(h, hipMemcpyAsync(h->d_key[0], ref_ids, n * 4, hipMemcpyHostToDevice, h->stream));
    if ((rc = mkc_time_begin(h))) return rc;
    hipLaunchKernelGGL(mkc_gid_kernel, dim3(mkc_blocks(h, n)), dim3(MKC_BLOCK), 0, h->stream, (const unsigned long long *)h->d_index, R, n, h->d_val[0]);
    MKC_HIP(h, hipGetLastError());
    int w = 0;
    MKC_HIP(h, mkc_sort(h, h->d_key, h->d_val, n, &w));
    /* row heads */
    mkc_row_f f{h->d_key[w], nullptr, nullptr, 0};
    if ((rc = mkc_compact_count(h, f, n, nullptr, h->d_base))) return rc;
    uint64_t nrows = 0;
    if ((rc = mkc_fetch_word(h, h->d_base, &nrows))) return rc;
    cap = 0;
    if ((rc = mkc_grow(h, &c.d_row_ids, &cap, nrows, false))) return rc;
    cap = 0;
    if ((rc = mkc_grow(h, &c.d_row_start, &cap, nrows + 1, false))) return rc;
    cap = 0;
    if ((rc = mkc_grow(h, &c.d_refs, &cap, n, false))) return rc;
    f.row_ids = c.d_row_ids; f.row_start = c.d_row_start; f.cap = nrows;
    if ((rc = mkc_compact_emit(h, f, n))) return rc;
    hipLaunchKernelGGL(mkc_set_u32_kernel, dim3(1), dim3(1), 0, h->stream, c.d_row_start + nrows, (uint32_t)n);
    MKC_HIP(h, hipGetLastError());
    MKC_HIP(h, hipMemcpyAsync(c.d_refs, h->d_val[w], n * 4, hipMemcpyDeviceToDevice, h->stream));
    /* the largest id decides how many high bits a bucket number takes */
    uint32_t *h_max = (uint32_t *)(h->h_word + 1);
    MKC_HIP(h, hipMemcpyAsync(h_max, c.d_row_ids + (nrows - 1), 4, hipMemcpyDeviceToHost, h->stream));
    MKC_HIP(h, hipStreamSynchronize(h->stream));
    const uint32_t maxid = *h_max;
    uint32_t idbits = 0, rowbits = 0;
    while (idbits < 32u && ((uint64_t)maxid >> idbits)) idbits++;
    while (rowbits < MKC_BUCKET_BITS && (1ull << rowbits) < nrows) rowbits++;
    c.shift = idbits > rowbits ? idbits - rowbits : 0u;
    c.nbuckets = (uint32_t)(((uint64_t)maxid >> c.shift) + 1u);
    cap = 0;
    if ((rc = mkc_grow(h, &c.d_bucket, &cap, (uint64_t)c.nbuckets + 1, false))) return rc;
    hipLaunchKernelGGL(mkc_bucket_kernel, dim3((unsigned)(((uint64_t)c.nbuckets + 1 + MKC_BLOCK - 1) / MKC_BLOCK)), dim3(MKC_BLOCK), 0, h->stream,
                       (const uint32_t *)c.d_row_ids, nrows, c.shift, c.nbuckets, c.d_bucket);
    MKC_HIP(h, hipGetLastError());
    if ((rc = mkc_time_end(h, &h->load_ms))) return rc;
    c.nrows = nrows;
  }
  c.loaded = true;
  return MK_OK;
}

extern "C" int mk_composite_query_begin(mk_composite *h, uint32_t nsamples) {
  if (!h) return MK_ERR_ARG;
  if (!h->load_begun) return mkc_fail(h, MK_ERR_STATE, "mk_composite_query_begin before the database is loaded");
  for (uint32_t c = 0; c < h->comp_num; c++)
    if (!h->comp[c].loaded) return mkc_fail(h, MK_ERR_STATE, "mk_composite_query_begin: component %u of the database is not loaded", c);
  if (nsamples == 0xFFFFFFFFu) return mkc_fail(h, MK_ERR_ARG, "mk_composite_query_begin: fewer than 2^32 - 1 samples");
  MKC_HIP(h, hipSetDevice(h->device));
  int rc = mkc_grow(h, &h->d_sample_hits, &h->sample_cap, (uint64_t)nsamples + 1);
  if (rc) return rc;
  MKC_HIP(h, hipMemsetAsync(h->d_sample_hits, 0, ((size_t)nsamples + 1) * 8, h->stream));
  for (auto &c : h->comp) { c.have = false; c.nq = 0; }
  h->batch_kind = MKC_BATCH_NONE; h->next_k = 0;
  h->nsamples = nsamples;
  h->query_ms = 0.0;
  h->hits = 0; h->ranges = 0;
  h->querying = true;
  return MK_OK;
}

extern "C" int mk_composite_query_component(mk_composite *h, uint32_t ci, const uint32_t *ids, const uint16_t *counts, const uint64_t *index) {
  if (!h || !index) return MK_ERR_ARG;
  if (!h->load_begun || !h->querying) return mkc_fail(h, MK_ERR_STATE, "mk_composite_query_component before mk_composite_query_begin");
  if (ci >= h->comp_num) return mkc_fail(h, MK_ERR_ARG, "component %u of %u", ci, h->comp_num);
  if (h->batch_kind == MKC_BATCH_DEVICE) return mkc_fail(h, MK_ERR_STATE, "mk_composite_query_component in a batch fed by mk_composite_query_sample_keys");
  mkc_comp &c = h->comp[ci];
  if (c.have) return mkc_fail(h, MK_ERR_STATE, "component %u given twice in one batch", ci);
  const uint32_t S = h->nsamples;
  const uint64_t nq = index[S];
  if (nq && (!ids || !counts)) return MK_ERR_ARG;
  if (nq >= 0xFFFFFFFFull) return mkc_fail(h, MK_ERR_ARG, "mk_composite_query_component: a batch of %llu ids in one component (fewer than 2^32 - 1 are supported)", (unsigned long long)nq);
  if (index[0] != 0) return mkc_fail(h, MK_ERR_ARG, "the batch's positions do not start at 0");
  for (uint32_t j = 0; j < S; j++)
    if (index[j] > index[j + 1]) return mkc_fail(h, MK_ERR_ARG, "the batch's positions are not ascending at sample %u", j);
  MKC_HIP(h, hipSetDevice(h->device));
  try { c.qindex.assign(index, index + (size_t)S + 1); } catch (...) { return mkc_fail(h, MK_ERR_NOMEM, "out of memory"); }
  h->batch_kind = MKC_BATCH_HOST;
  c.have = true;
  c.nq = nq;
  if (nq == 0 || c.nrows == 0) { c.nq = 0; return MK_OK; } /* nothing of this component can hit */
  int rc;
  if ((rc = mkc_grow(h, &c.d_qids, &c.q_cap, nq))) return rc;
  if ((rc = mkc_grow(h, &c.d_qcnt, &c.qcnt_cap, nq))) return rc;
  if ((rc = mkc_grow(h, &c.d_rowidx, &c.rowidx_cap, nq))) return rc;
  if ((rc = mkc_grow(h, &c.d_qindex, &c.qindex_cap, (uint64_t)S + 1))) return rc;
  uint64_t slots = 1024;
  while (slots < 2 * nq) slots <<= 1;
  if ((rc = mkc_grow(h, &h->d_tkey, &h->tkey_cap, slots, false))) return rc;
  if ((rc = mkc_grow(h, &h->d_tpos, &h->tpos_cap, slots, false))) return rc;
  MKC_HIP(h, hipMemcpyAsync(c.d_qids, ids, nq * 4, hipMemcpyHostToDevice, h->stream));
  MKC_HIP(h, hipMemcpyAsync(c.d_qcnt, counts, nq * 2, hipMemcpyHostToDevice, h->stream));
  MKC_HIP(h, hipMemcpyAsync(c.d_qindex, index, ((size_t)S + 1) * 8, hipMemcpyHostToDevice, h->stream));
  if ((rc = mkc_time_begin(h))) return rc;
  MKC_HIP(h, hipMemsetAsync(h->d_tkey, 0xFF, slots * 8, h->stream));
  MKC_HIP(h, hipMemsetAsync(h->d_tpos, 0xFF, slots * 4, h->stream));
  hipLaunchKernelGGL(mkc_lookup_kernel<false>, dim3(mkc_blocks(h, nq)), dim3(MKC_BLOCK), 0, h->stream, (const uint32_t *)c.d_qids, nq,
                     (const unsigned long long *)c.d_qindex, S, (const uint32_t *)c.d_row_ids, (const uint32_t *)c.d_bucket, c.shift, c.nbuckets,
                     h->d_tkey, h->d_tpos, slots - 1, c.d_rowidx);
  hipLaunchKernelGGL(mkc_winner_kernel<false>, dim3(mkc_blocks(h, nq)), dim3(MKC_BLOCK), 0, h->stream, (const uint32_t *)c.d_qids, nq,
                     (const unsigned long long *)c.d_qindex, S, (const uint32_t *)c.d_row_start, (const unsigned long long *)h->d_tkey,
                     (const uint32_t *)h->d_tpos, slots - 1, c.d_rowidx, h->d_sample_hits);
  MKC_HIP(h, hipGetLastError());
  if ((rc = mkc_time_end(h, &h->query_ms))) return rc; /* (waits: the caller's arrays are free again) */
  return MK_OK;
}

/* a query array that grows and keeps its first `keep` entries (the samples a device-fed batch has taken already) */
template <class T>
static int mkc_grow_keep(mk_composite *h, T **p, uint64_t *cap, uint64_t need, uint64_t keep) {
  if (need <= *cap && *p) return MK_OK;
  T *np = nullptr;
  const uint64_t c = need + need / 2 + 1024;
  hipError_t r = mk_dev_alloc((void **)&np, c * sizeof(T));
  if (r != hipSuccess) return mkc_fail(h, MK_ERR_NOMEM, "device allocation of %llu bytes: %s", (unsigned long long)(c * sizeof(T)), hipGetErrorString(r));
  if (keep && *p) {
    r = hipMemcpyAsync(np, *p, keep * sizeof(T), hipMemcpyDeviceToDevice, h->stream);
    if (r == hipSuccess) r = hipStreamSynchronize(h->stream); /* the old array goes now */
    if (r != hipSuccess) { (void)hipFree(np); return mkc_fail(h, MK_ERR_HIP, "copying a query array: %s", hipGetErrorString(r)); }
  }
  (void)hipFree(*p);
  *p = np; *cap = c;
  return MK_OK;
}

extern "C" int mk_composite_query_sample_keys(mk_composite *h, uint32_t k, const uint64_t *keys_dev, const uint32_t *counts_dev, uint64_t n,
                                              uint32_t comp_code_bits) {
  if (!h) return MK_ERR_ARG;
  if (!h->load_begun || !h->querying) return mkc_fail(h, MK_ERR_STATE, "mk_composite_query_sample_keys before mk_composite_query_begin");
  if (h->batch_kind == MKC_BATCH_HOST) return mkc_fail(h, MK_ERR_STATE, "mk_composite_query_sample_keys in a batch fed by mk_composite_query_component");
  const uint32_t C = h->comp_num;
  if (C > MKC_PART_MAX) return mkc_fail(h, MK_ERR_ARG, "mk_composite_query_sample_keys: %u components (at most %u are supported)", C, MKC_PART_MAX);
  if (comp_code_bits >= 32u || (1u << comp_code_bits) != C)
    return mkc_fail(h, MK_ERR_ARG, "mk_composite_query_sample_keys: comp_code_bits %u does not go with the database's %u components", comp_code_bits, C);
  if (k != h->next_k || k >= h->nsamples)
    return mkc_fail(h, MK_ERR_ARG, "mk_composite_query_sample_keys: sample %u, expected %u of %u (samples come in ascending order)", k, h->next_k, h->nsamples);
  if (n && (!keys_dev || !counts_dev)) return MK_ERR_ARG;
  if (n >= 0xFFFFFFFFull) return mkc_fail(h, MK_ERR_ARG, "mk_composite_query_sample_keys: a sample of %llu keys (fewer than 2^32 - 1 are supported)", (unsigned long long)n);
  MKC_HIP(h, hipSetDevice(h->device));
  if (h->batch_kind == MKC_BATCH_NONE) /* positions of the samples taken so far, per component: [0] */
    try { for (auto &c : h->comp) c.qindex.assign(1, 0); } catch (...) { return mkc_fail(h, MK_ERR_NOMEM, "out of memory"); }
  h->batch_kind = MKC_BATCH_DEVICE;
  int rc;
  if (n) {
    if ((rc = mkc_time_begin(h))) return rc;
    MKC_HIP(h, hipMemsetAsync(h->d_part, 0, 2 * MKC_PART_MAX * sizeof(unsigned long long), h->stream));
    hipLaunchKernelGGL(mkc_part_count_kernel, dim3(mkc_blocks(h, n)), dim3(MKC_BLOCK), 0, h->stream, (const unsigned long long *)keys_dev, n, C, h->d_part);
    MKC_HIP(h, hipGetLastError());
    MKC_HIP(h, hipMemcpyAsync(h->h_part, h->d_part, MKC_PART_MAX * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    MKC_HIP(h, hipStreamSynchronize(h->stream));
    uint64_t sum = 0;
    for (uint32_t ci = 0; ci < C; ci++) sum += h->h_part[ci];
    if (sum != n) return mkc_fail(h, MK_ERR_STATE, "mk_composite_query_sample_keys: %llu keys counted, %llu given", (unsigned long long)sum, (unsigned long long)n);
    mkc_part_dst dst{};
    for (uint32_t ci = 0; ci < C; ci++) {
      mkc_comp &c = h->comp[ci];
      const uint64_t need = c.nq + h->h_part[ci];
      if (need >= 0xFFFFFFFFull) return mkc_fail(h, MK_ERR_ARG, "mk_composite_query_sample_keys: a batch of %llu ids in one component (fewer than 2^32 - 1 are supported)", (unsigned long long)need);
      if (need) {
        if ((rc = mkc_grow_keep(h, &c.d_qids, &c.q_cap, need, c.nq))) return rc;
        if ((rc = mkc_grow_keep(h, &c.d_qcnt, &c.qcnt_cap, need, c.nq))) return rc;
      }
      dst.qids[ci] = c.d_qids; dst.qcnt[ci] = c.d_qcnt; dst.base[ci] = c.nq; dst.cap[ci] = need;
    }
    hipLaunchKernelGGL(mkc_part_scatter_kernel, dim3(mkc_blocks(h, n)), dim3(MKC_BLOCK), 0, h->stream, (const unsigned long long *)keys_dev, counts_dev, n, C,
                       comp_code_bits, h->d_part + MKC_PART_MAX, dst);
    MKC_HIP(h, hipGetLastError());
    if ((rc = mkc_time_end(h, &h->query_ms))) return rc; /* (waits for the handle's stream: the caller's list has been read) */
    for (uint32_t ci = 0; ci < C; ci++) h->comp[ci].nq += h->h_part[ci];
  }
  try { for (auto &c : h->comp) c.qindex.push_back(c.nq); } catch (...) { return mkc_fail(h, MK_ERR_NOMEM, "out of memory"); }
  h->next_k = k + 1;
  return MK_OK;
}

/* a device-fed batch is complete: per component the positions of its samples go up and every position finds its row; no table */
static int mkc_lookup_distinct(mk_composite *h) {
  const uint32_t S = h->nsamples;
  int rc;
  if ((rc = mkc_time_begin(h))) return rc;
  for (auto &c : h->comp) {
    c.have = c.nq != 0;
    if (!c.have) continue;
    try { c.qindex.resize((size_t)S + 1, c.nq); } catch (...) { return mkc_fail(h, MK_ERR_NOMEM, "out of memory"); } /* samples that never came are empty */
    if ((rc = mkc_grow(h, &c.d_rowidx, &c.rowidx_cap, c.nq))) return rc;
    if ((rc = mkc_grow(h, &c.d_qindex, &c.qindex_cap, (uint64_t)S + 1))) return rc;
    MKC_HIP(h, hipMemcpyAsync(c.d_qindex, c.qindex.data(), ((size_t)S + 1) * 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(mkc_lookup_kernel<true>, dim3(mkc_blocks(h, c.nq)), dim3(MKC_BLOCK), 0, h->stream, (const uint32_t *)c.d_qids, c.nq,
                       (const unsigned long long *)c.d_qindex, S, (const uint32_t *)c.d_row_ids, (const uint32_t *)c.d_bucket, c.shift, c.nbuckets,
                       (unsigned long long *)nullptr, (uint32_t *)nullptr, (uint64_t)0, c.d_rowidx);
    hipLaunchKernelGGL(mkc_winner_kernel<true>, dim3(mkc_blocks(h, c.nq)), dim3(MKC_BLOCK), 0, h->stream, (const uint32_t *)c.d_qids, c.nq,
                       (const unsigned long long *)c.d_qindex, S, (const uint32_t *)c.d_row_start, (const unsigned long long *)nullptr,
                       (const uint32_t *)nullptr, (uint64_t)0, c.d_rowidx, h->d_sample_hits);
    MKC_HIP(h, hipGetLastError());
  }
  /* (the copies above read the host vectors: waited for before anyone may change them) */
  return mkc_time_end(h, &h->query_ms);
}

/* samples [s0, s1) with `tot` hits between them: their rows, in (sample, reference) order, appended to h->rows / h->row_sample */
static int mkc_run_range(mk_composite *h, uint32_t s0, uint32_t s1, uint64_t tot) {
  int rc;
  if ((rc = mkc_grow_pairs(h, tot))) return rc;
  MKC_HIP(h, hipMemsetAsync(h->d_base, 0, 8, h->stream));
  uint32_t k = 0;
  for (uint32_t ci = 0; ci < h->comp_num; ci++) {
    mkc_comp &c = h->comp[ci];
    if (!c.have || c.nq == 0) continue;
    const uint64_t p0 = c.qindex[s0], n = c.qindex[s1] - p0;
    if (n == 0) continue;
    mkc_hit_f f{c.d_rowidx, c.d_row_start, c.d_refs, c.d_qcnt, c.d_qindex, h->nsamples, s0, h->ref_num, p0, tot, h->d_key[0], h->d_val[0]};
    if ((rc = mkc_compact_count(h, f, n, h->d_base + k, h->d_base + k + 1))) return rc;
    if ((rc = mkc_compact_emit(h, f, n))) return rc;
    k++;
  }
  uint64_t got = 0;
  if ((rc = mkc_fetch_word(h, h->d_base + k, &got))) return rc;
  if (got != tot) return mkc_fail(h, MK_ERR_STATE, "samples %u..%u: %llu hits emitted, %llu counted", s0, s1 - 1, (unsigned long long)got, (unsigned long long)tot);
  /* by count, then stably by segment: a segment's counts ascend */
  int w = 0;
  MKC_HIP(h, mkc_sort(h, h->d_key, h->d_val, tot, &w));
  uint32_t *k2[2] = {h->d_val[w], h->d_val[w ^ 1]}, *v2[2] = {h->d_key[w], h->d_key[w ^ 1]};
  int w2 = 0;
  MKC_HIP(h, mkc_sort(h, k2, v2, tot, &w2));
  const uint32_t *seg = k2[w2], *cnt = v2[w2];
  uint64_t nseg = 0, nbig = 0;
  mkc_head_f hf{seg, nullptr, 0};
  if ((rc = mkc_compact_count(h, hf, tot, nullptr, h->d_base))) return rc;
  if ((rc = mkc_fetch_word(h, h->d_base, &nseg))) return rc;
  if ((rc = mkc_grow(h, &h->d_starts, &h->starts_cap, nseg))) return rc;
  hf.starts = h->d_starts; hf.cap = nseg;
  if ((rc = mkc_compact_emit(h, hf, tot))) return rc;
  mkc_big_f bf{h->d_starts, nseg, tot, 0, nullptr};
  if ((rc = mkc_compact_count(h, bf, nseg, nullptr, h->d_base))) return rc;
  if ((rc = mkc_fetch_word(h, h->d_base, &nbig))) return rc;
  if (nbig == 0) return MK_OK;
  if ((rc = mkc_grow(h, &h->d_big, &h->big_cap, nbig))) return rc;
  bf.big = h->d_big; bf.cap = nbig;
  if ((rc = mkc_compact_emit(h, bf, nseg))) return rc;
  if ((rc = mkc_grow(h, &h->d_rows, &h->rows_cap, nbig))) return rc;
  if (nbig > h->h_rows_cap || !h->h_rows) {
    if (h->h_rows) (void)hipHostFree(h->h_rows);
    h->h_rows = nullptr; h->h_rows_cap = 0;
    const uint64_t cap = nbig + nbig / 8 + 1024;
    MKC_HIP(h, mk_pin_alloc((void **)&h->h_rows, cap * sizeof(mk_composite_row), hipHostMallocDefault));
    h->h_rows_cap = cap;
  }
  hipLaunchKernelGGL(mkc_stats_kernel, dim3((unsigned)((nbig + MKC_BLOCK / 64 - 1) / (MKC_BLOCK / 64))), dim3(MKC_BLOCK), 0, h->stream, seg, cnt,
                     (const uint32_t *)h->d_starts, nseg, tot, (const uint32_t *)h->d_big, nbig, h->d_rows);
  MKC_HIP(h, hipGetLastError());
  MKC_HIP(h, hipMemcpyAsync(h->h_rows, h->d_rows, nbig * sizeof(mk_composite_row), hipMemcpyDeviceToHost, h->stream));
  MKC_HIP(h, hipStreamSynchronize(h->stream));
  try {
    for (uint64_t i = 0; i < nbig; i++) {
      mk_composite_row r = h->h_rows[i];
      const uint32_t segno = r.ref;
      r.ref = segno % h->ref_num;
      h->rows.push_back(r);
      h->row_sample.push_back(s0 + segno / h->ref_num);
    }
  } catch (...) { return mkc_fail(h, MK_ERR_NOMEM, "out of memory"); }
  return MK_OK;
}

extern "C" int mk_composite_query_finish(mk_composite *h, const mk_composite_row **rows, uint64_t *row_end) {
  if (!h || !rows || (h->nsamples && !row_end)) return MK_ERR_ARG;
  if (!h->load_begun || !h->querying) return mkc_fail(h, MK_ERR_STATE, "mk_composite_query_finish before mk_composite_query_begin");
  MKC_HIP(h, hipSetDevice(h->device));
  h->querying = false;
  const uint32_t S = h->nsamples, R = h->ref_num;
  h->rows.clear();
  h->row_sample.clear();
  *rows = nullptr;
  if (S == 0) return MK_OK;
  if (h->batch_kind == MKC_BATCH_DEVICE) {
    const int lrc = mkc_lookup_distinct(h);
    if (lrc) return lrc;
  }
  if (S > h->h_sample_cap || !h->h_sample_hits) {
    if (h->h_sample_hits) (void)hipHostFree(h->h_sample_hits);
    h->h_sample_hits = nullptr; h->h_sample_cap = 0;
    MKC_HIP(h, mk_pin_alloc((void **)&h->h_sample_hits, ((size_t)S + 1024) * 8, hipHostMallocDefault));
    h->h_sample_cap = (uint64_t)S + 1024;
  }
  MKC_HIP(h, hipMemcpyAsync(h->h_sample_hits, h->d_sample_hits, (size_t)S * 8, hipMemcpyDeviceToHost, h->stream));
  MKC_HIP(h, hipStreamSynchronize(h->stream));
  const unsigned long long *sh = h->h_sample_hits;
  int rc;
  if ((rc = mkc_time_begin(h))) return rc;
  for (uint32_t s0 = 0; s0 < S;) {
    uint32_t s1 = s0;
    uint64_t tot = 0;
    while (s1 < S) {
      if (s1 > s0 && (tot + sh[s1] > h->max_hits || (uint64_t)(s1 - s0 + 1) * R > 0xFFFFFFFFull)) break;
      tot += sh[s1];
      s1++;
    }
    /* one sample above the capacity: the buffer grows (it never truncates); the sort takes fewer than 2^32 pairs */
    if (tot >= (1ull << 32))
      return mkc_fail(h, MK_ERR_ARG, "sample %u of the batch alone has %llu hits (fewer than 2^32 are supported)", s0, (unsigned long long)tot);
    if (tot) {
      if ((rc = mkc_run_range(h, s0, s1, tot))) {
        if (rc == MK_ERR_NOMEM && s1 == s0 + 1) {
          char msg[200];
          snprintf(msg, sizeof msg, "%s", h->err);
          return mkc_fail(h, MK_ERR_NOMEM, "sample %u of the batch (%llu hits): %.150s", s0, (unsigned long long)tot, msg);
        }
        return rc;
      }
      h->hits += tot;
      h->ranges++;
    }
    s0 = s1;
  }
  if ((rc = mkc_time_end(h, &h->query_ms))) return rc;
  /* rows are in (sample, reference) order: per sample, kmer_num descending, stable */
  size_t i = 0;
  for (uint32_t s = 0; s < S; s++) {
    const size_t a = i;
    while (i < h->rows.size() && h->row_sample[i] == s) i++;
    std::stable_sort(h->rows.begin() + a, h->rows.begin() + i, [](const mk_composite_row &x, const mk_composite_row &y) { return x.kmer_num > y.kmer_num; });
    row_end[s] = i;
  }
  *rows = h->rows.data();
  return MK_OK;
}

extern "C" int mk_composite_last_kernel_ms(mk_composite *h, double *load_ms, double *query_ms) {
  if (!h || !load_ms || !query_ms) return MK_ERR_ARG;
  *load_ms = h->load_ms;
  *query_ms = h->query_ms;
  return MK_OK;
}

extern "C" int mk_composite_last_counts(mk_composite *h, uint64_t *hits, uint64_t *ranges) {
  if (!h || !hits || !ranges) return MK_ERR_ARG;
  *hits = h->hits;
  *ranges = h->ranges;
  return MK_OK;
}
