/*
 * mk_abv.hip -- the abundance-vector index and search of `composite -i` / `composite -s` on the device (gfx950, hand-written).
 *
 * index_abv() (command_composite.c:347-440) turns the sample-major .abv files (binVec_t {ref_idx, pct}, command_composite.h:12-16)
 * into a species-major matrix: for every species, the (file number, pct) of every file entry that names it, appended file by
 * file (abundance_Vec.abm), the cumulative counts over the species (.abmi) and one norm per file (.yl2n).  abv_search()
 * (:212-344) walks, for every entry d of a query vector in file order, the column of its species and accumulates a float
 * measure per sample, then qsort()s the matched samples by it (comparator_measure, :660-665).
 *
 *   mk_abv_prep_kernel     (species, position) pairs; the first entry whose species is outside 0..nref-1 (atomicMin)
 *   mk_radix_sort_pairs_u32 (mk_sort.hip.h)   by species, STABLE: within a species, by file, then by position in the file --
 *                          the append order of the reference's realloc loop (:390-398)
 *   mk_abv_gather_kernel   .abm: {file number (binary search in the file ends), pct}
 *   mk_abv_abmi_kernel     .abmi: entries with species <= r (binary search in the sorted species)
 *   mk_abv_yl2n_kernel     one thread per file: the sequential double sum of (float)(pct * pct) (:385-387); sqrt on the host
 *   mk_abv_check_kernel    (load) every column ascends by sample and names samples below nsamples
 *   mk_abv_search_kernel   grid = tiles of 1024 samples x queries; a workgroup keeps its tile's accumulators in LDS, takes
 *                          the query's entries in order (a window of 256 binary searches at a time), and between entries
 *                          waits at a barrier: every sample is summed in the reference's order by one lane, no atomics.
 *                          A run of one sample inside a column (a file that lists a species twice) is summed by the lane
 *                          at its head.  Records the first entry that touched each sample and finishes the measure.
 *   mk_abv_scan_kernel / mk_abv_emit_kernel   ordered compaction of the matched samples, query-major
 *   three stable radix sorts (first entry, then the measure as an order-preserving u32 with -0 == +0, then the query):
 *                          discovery order (:261-265), then glibc 2.35's stable merge-sort qsort by the measure
 *   mk_abv_out_kernel      samples + measures in print order (cosine reversed, :329-331)
 * A query whose measures hold a NaN makes comparator_measure inconsistent; that query is sorted on the host by an exact
 * restatement of glibc's msort_with_tmp (n1 = n / 2, ties from the left).
 *
 * Float arithmetic is the reference's (gcc on x86-64 without -mfma does not contract): no contraction in this file.
 */
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include "mk_poison.hip.h"

namespace { /* mk_mco.hip holds the sort's kernels too: this file's copies stay local */
#include "mk_sort.hip.h"
}

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "metakssd_hip.h"

#define MK_ABV_TILE 1024u    /* samples per search workgroup: m, x, y, first in LDS = 16 KiB */
#define MK_ABV_THREADS 256u
#define MK_ABV_WIN 256u      /* query entries whose column ranges are looked up together */
#define MK_ABV_UNSET 0xFFFFFFFFu

struct mk_abv {
  int device = 0, num_cu = 256;
  hipStream_t stream = nullptr;
  /* index */
  mk_binvec *d_in = nullptr;
  uint64_t in_cap = 0;
  uint32_t *d_key[2] = {nullptr, nullptr}, *d_val[2] = {nullptr, nullptr};
  uint64_t pair_cap[4] = {0, 0, 0, 0};
  void *d_tmp = nullptr; /* radix sort: histograms, totals, flags */
  uint32_t *h_sort_flag = nullptr;
  unsigned long long *d_fend = nullptr;
  uint64_t fend_cap = 0;
  mk_binvec *d_abm = nullptr;
  uint64_t abm_cap = 0;
  int32_t *d_abmi = nullptr;
  uint64_t abmi_cap = 0;
  double *d_ysum = nullptr;
  uint64_t ysum_cap = 0;
  uint32_t *d_bad = nullptr, *h_bad = nullptr;
  mk_binvec *h_abm = nullptr;
  int32_t *h_abmi = nullptr;
  double *h_yl2n = nullptr;
  uint64_t h_abm_cap = 0, h_abmi_cap = 0, h_yl2n_cap = 0;
  /* loaded index */
  bool loaded = false;
  uint32_t *d_col_s = nullptr;
  float *d_col_p = nullptr;
  uint64_t col_cap[2] = {0, 0}, n = 0;
  int32_t *d_lidx = nullptr;
  uint64_t lidx_cap = 0;
  double *d_yl2n = nullptr;
  uint64_t yl2n_cap = 0;
  uint32_t nref = 0, nsamples = 0;
  /* search */
  mk_binvec *d_q = nullptr;
  uint64_t q_cap = 0;
  unsigned long long *d_qoff = nullptr;
  double *d_qnorm = nullptr;
  uint32_t *d_nan = nullptr;
  uint64_t qn_cap[3] = {0, 0, 0};
  uint32_t *d_first = nullptr;
  float *d_meas = nullptr;
  uint64_t dense_cap[2] = {0, 0};
  uint32_t *d_tcnt = nullptr;
  unsigned long long *d_toff = nullptr;
  uint64_t t_cap[2] = {0, 0};
  uint32_t *d_ef = nullptr, *d_es = nullptr, *d_eq = nullptr;
  float *d_em = nullptr;
  uint64_t e_cap[4] = {0, 0, 0, 0};
  int32_t *d_os = nullptr;
  float *d_om = nullptr;
  uint32_t *d_of = nullptr;
  uint64_t o_cap[3] = {0, 0, 0};
  int32_t *h_os = nullptr;
  float *h_om = nullptr;
  uint64_t h_o_cap[2] = {0, 0};
  unsigned long long *h_toff = nullptr;
  uint64_t h_toff_cap = 0;
  uint32_t *h_nan = nullptr;
  uint64_t h_nan_cap = 0;
  /* mk_abv_last_kernel_ms */
  hipEvent_t ev_index[2] = {nullptr, nullptr}, ev_search[2] = {nullptr, nullptr};
  bool index_timed = false, search_timed = false;
  char err[256] = {0};
};

static thread_local char mk_abv_create_err[256];

static int mk_abv_fail(mk_abv *a, int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(a ? a->err : mk_abv_create_err, 256, fmt, ap);
  va_end(ap);
  return code;
}

#define MK_ABV_HIP(a, call)                                                                          \
  do {                                                                                               \
    hipError_t _r = (call);                                                                          \
    if (_r != hipSuccess) return mk_abv_fail(a, MK_ERR_HIP, "%s: %s", #call, hipGetErrorString(_r)); \
  } while (0)

template <class T>
static int mk_abv_grow(mk_abv *a, T **p, uint64_t *cap, uint64_t need) {
  if (need == 0) need = 1;
  if (need <= *cap && *p) return MK_OK;
  (void)hipFree(*p);
  *p = nullptr; *cap = 0;
  const uint64_t c = need + need / 8 + 256;
  MK_ABV_HIP(a, mk_dev_alloc((void **)p, c * sizeof(T)));
  *cap = c;
  return MK_OK;
}

template <class T>
static int mk_abv_grow_pinned(mk_abv *a, T **p, uint64_t *cap, uint64_t need) {
  if (need == 0) need = 1;
  if (need <= *cap && *p) return MK_OK;
  if (*p) (void)hipHostFree(*p);
  *p = nullptr; *cap = 0;
  const uint64_t c = need + need / 8 + 256;
  MK_ABV_HIP(a, mk_pin_alloc((void **)p, c * sizeof(T), hipHostMallocDefault));
  *cap = c;
  return MK_OK;
}

static unsigned mk_abv_blocks(const mk_abv *a, uint64_t n, unsigned per_block) {
  uint64_t b = (n + per_block - 1) / per_block;
  const uint64_t cap = (uint64_t)a->num_cu * 32u;
  if (b > cap) b = cap;
  return b ? (unsigned)b : 1u;
}

/* ---- kernels ------------------------------------------------------------------------------------------ */

/* first position in a[lo, hi) whose value is >= x (a ascending) */
template <class T, class X>
__device__ __forceinline__ uint64_t mk_abv_lower(const T *a, uint64_t lo, uint64_t hi, X x) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if ((X)a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

/* first position in a[lo, hi) whose value is > x */
template <class T, class X>
__device__ __forceinline__ uint64_t mk_abv_upper(const T *a, uint64_t lo, uint64_t hi, X x) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if ((X)a[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(256) mk_abv_prep_kernel(const mk_binvec *in, uint64_t n, uint32_t nref, uint32_t *key, uint32_t *val,
                                                          uint32_t *bad) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const int32_t r = in[i].ref_idx;
    if (r < 0 || (uint32_t)r >= nref) atomicMin(bad, (uint32_t)i); /* the reference writes out of bounds here (:390-397) */
    key[i] = (uint32_t)r;
    val[i] = (uint32_t)i;
  }
}

/* :393-394: the entry at position pos of the concatenation belongs to file f with fend[f - 1] <= pos < fend[f] */
__global__ void __launch_bounds__(256) mk_abv_gather_kernel(const mk_binvec *in, const uint32_t *pos, uint64_t n, const unsigned long long *fend,
                                                            uint32_t nfiles, mk_binvec *abm) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t p = pos[i];
    mk_binvec o;
    o.ref_idx = (int32_t)mk_abv_upper(fend, 0, nfiles, (unsigned long long)p);
    o.pct = in[p].pct;
    abm[i] = o;
  }
}

/* :420-421: the cumulative counts = entries whose species is <= r */
__global__ void __launch_bounds__(256) mk_abv_abmi_kernel(const uint32_t *skey, uint64_t n, uint32_t nref, int32_t *abmi) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nref; r += (uint64_t)gridDim.x * blockDim.x)
    abmi[r] = (int32_t)mk_abv_upper(skey, 0, n, (uint32_t)r);
}

/* :385-387: y_l2n += binVec_tmp.pct * binVec_tmp.pct -- a float product added to a double, in file order */
__global__ void __launch_bounds__(256) mk_abv_yl2n_kernel(const mk_binvec *in, const unsigned long long *fend, uint32_t nfiles, double *ysum) {
  for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < nfiles; f += (uint64_t)gridDim.x * blockDim.x) {
    double y = 0.0;
    for (uint64_t i = f ? fend[f - 1] : 0; i < fend[f]; i++) {
      const float p = in[i].pct;
      const float pp = p * p;
      y += (double)pp;
    }
    ysum[f] = y;
  }
}

/* load: the interleaved matrix into two arrays */
__global__ void __launch_bounds__(256) mk_abv_split_kernel(const mk_binvec *abm, uint64_t n, uint32_t *col_s, float *col_p) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const mk_binvec e = abm[i];
    col_s[i] = (uint32_t)e.ref_idx;
    col_p[i] = e.pct;
  }
}

/* load: what the search relies on -- a column's samples ascend (an index made by -i) and lie below nsamples */
__global__ void __launch_bounds__(256) mk_abv_check_kernel(const uint32_t *col_s, const int32_t *abmi, uint32_t nref, uint32_t nsamples,
                                                           uint32_t *bad) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nref; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t lo = r ? (uint64_t)abmi[r - 1] : 0, hi = (uint64_t)abmi[r];
    uint32_t prev = 0;
    for (uint64_t j = lo; j < hi; j++) {
      const uint32_t s = col_s[j];
      if (s >= nsamples || s < prev) { atomicMin(bad, (uint32_t)r); break; }
      prev = s;
    }
  }
}

/* (float)(m / den) with x86-64's NaN: 0/0 (an all-zero vector) gives the default NaN, whose sign bit is set ("-nan" in the
 * reference's output); a NaN operand is passed on, the numerator's first.  double -> float keeps the sign and the high payload */
__device__ __forceinline__ float mk_abv_cosine(float m, double den) {
  const double num = (double)m, r = num / den;
  if (r == r) return (float)r;
  const unsigned long long b = num != num ? __double_as_longlong(num) : den != den ? __double_as_longlong(den) : 0xFFF8000000000000ull;
  return __uint_as_float(((uint32_t)(b >> 32) & 0x80000000u) | 0x7FC00000u | ((uint32_t)(b >> 29) & 0x003FFFFFu));
}

/* abv_search() :262-285 for one tile of samples and one query; the finish of :287-310 */
template <int METRIC>
__global__ void __launch_bounds__(MK_ABV_THREADS) mk_abv_search_kernel(const uint32_t *col_s, const float *col_p, const int32_t *abmi,
                                                                       const double *yl2n, uint32_t S, uint32_t ntiles, const mk_binvec *q,
                                                                       const unsigned long long *qoff, const double *qnorm,
                                                                       uint32_t *first_out, float *meas_out, uint32_t *tile_cnt,
                                                                       uint32_t *nan_flag) {
  __shared__ float am[MK_ABV_TILE], ax[MK_ABV_TILE], ay[MK_ABV_TILE];
  __shared__ uint32_t af[MK_ABV_TILE];
  __shared__ uint32_t wlo[MK_ABV_WIN], whi[MK_ABV_WIN];
  __shared__ float wx[MK_ABV_WIN];
  __shared__ uint32_t wsum[MK_ABV_THREADS / 64];
  const uint32_t t = threadIdx.x, tile = blockIdx.x, qi = blockIdx.y;
  const uint32_t s0 = tile * MK_ABV_TILE, s1 = S - s0 < MK_ABV_TILE ? S : s0 + MK_ABV_TILE;
  for (uint32_t i = t; i < MK_ABV_TILE; i += MK_ABV_THREADS) { am[i] = 0.f; ax[i] = 0.f; ay[i] = 0.f; af[i] = MK_ABV_UNSET; }
  const uint64_t q0 = qoff[qi], nd = qoff[qi + 1] - q0;
  for (uint64_t d0 = 0; d0 < nd; d0 += MK_ABV_WIN) {
    __syncthreads(); /* the LDS initialisation / the previous window's last step */
    if (t < MK_ABV_WIN && d0 + t < nd) { /* this window's column ranges, all lookups in flight together */
      const mk_binvec e = q[q0 + d0 + t];
      const int32_t r = e.ref_idx; /* 0 <= r < nref: checked on the host */
      const uint64_t cs = r ? (uint64_t)abmi[r - 1] : 0, ce = (uint64_t)abmi[r];
      const uint64_t lo = mk_abv_lower(col_s, cs, ce, s0);
      wlo[t] = (uint32_t)lo;
      whi[t] = (uint32_t)mk_abv_lower(col_s, lo, ce, s1);
      wx[t] = e.pct;
    }
    __syncthreads();
    const uint32_t kn = nd - d0 < MK_ABV_WIN ? (uint32_t)(nd - d0) : MK_ABV_WIN;
    for (uint32_t k = 0; k < kn; k++) {
      const uint32_t lo = wlo[k], hi = whi[k];
      const float xp = wx[k];
      for (uint32_t j = lo + t; j < hi; j += MK_ABV_THREADS) {
        const uint32_t s = col_s[j];
        if (j > lo && col_s[j - 1] == s) continue; /* not the head of its run */
        if (s < s0 || s >= s1) continue;          /* (cannot happen after the load check) */
        const uint32_t ls = s - s0;
        float m = am[ls], x = ax[ls], y = ay[ls];
        for (uint32_t jj = j; jj < hi && col_s[jj] == s; jj++) {
          const float yp = col_p[jj];
          if (METRIC == 1) { /* :268-271 */
            m += fabsf(yp - xp);
            x += xp;
            y += yp;
          } else if (METRIC == 2) { /* :273-274 */
            const float dd = yp - xp;
            m += dd * dd;
          } else { /* :275-276 */
            m += yp * xp;
          }
        }
        am[ls] = m;
        if (METRIC == 1) { ax[ls] = x; ay[ls] = y; }
        if (af[ls] == MK_ABV_UNSET) af[ls] = (uint32_t)(d0 + k); /* :262-266 */
      }
      __syncthreads();
    }
  }
  __syncthreads();
  uint32_t cnt = 0, nan = 0;
  const uint64_t base = (uint64_t)qi * S;
  for (uint32_t i = t; i < s1 - s0; i += MK_ABV_THREADS) {
    const uint32_t f = af[i];
    if (f != MK_ABV_UNSET) {
      float v = am[i];
      if (METRIC == 1) v = v + ((200.0f - ax[i]) - ay[i]);                     /* :300-301 */
      else if (METRIC == 0) v = mk_abv_cosine(v, qnorm[qi] * yl2n[s0 + i]);   /* :288-291 */
      meas_out[base + s0 + i] = v;
      cnt++;
      nan |= v != v ? 1u : 0u;
    }
    first_out[base + s0 + i] = f;
  }
  if (__any(nan)) { if ((t & 63u) == 0) atomicOr(&nan_flag[qi], 1u); }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
  if ((t & 63u) == 0) wsum[t >> 6] = cnt;
  __syncthreads();
  if (t == 0) {
    uint32_t c = 0;
    for (uint32_t w = 0; w < MK_ABV_THREADS / 64; w++) c += wsum[w];
    tile_cnt[(uint64_t)qi * ntiles + tile] = c;
  }
}

/* exclusive prefix of n counts (one workgroup, each thread a contiguous slice); off[n] = total */
__global__ void __launch_bounds__(1024) mk_abv_scan_kernel(const uint32_t *count, uint64_t n, unsigned long long *off) {
  __shared__ unsigned long long part[1024];
  const uint32_t t = threadIdx.x;
  const uint64_t per = (n + 1023u) / 1024u, lo = (uint64_t)t * per < n ? (uint64_t)t * per : n, hi = lo + per < n ? lo + per : n;
  unsigned long long sum = 0;
  for (uint64_t k = lo; k < hi; k++) sum += count[k];
  part[t] = sum;
  __syncthreads();
  for (uint32_t o = 1; o < 1024u; o <<= 1) {
    const unsigned long long v = t >= o ? part[t - o] : 0ull;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  unsigned long long run = part[t] - sum;
  for (uint64_t k = lo; k < hi; k++) { off[k] = run; run += count[k]; }
  if (t == 1023u) off[n] = part[t];
}

/* the matched samples of one (tile, query), in sample order, at the tile's offset: (first entry, measure, sample, query) and the
 * position as the sort's first value */
__global__ void __launch_bounds__(MK_ABV_THREADS) mk_abv_emit_kernel(const uint32_t *first, const float *meas, uint32_t S, uint32_t ntiles,
                                                                     const unsigned long long *toff, uint32_t *key, uint32_t *val, uint32_t *ef,
                                                                     float *em, uint32_t *es, uint32_t *eq) {
  __shared__ uint32_t wc[MK_ABV_THREADS / 64];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, tile = blockIdx.x, qi = blockIdx.y;
  const uint32_t s0 = tile * MK_ABV_TILE, s1 = S - s0 < MK_ABV_TILE ? S : s0 + MK_ABV_TILE;
  const uint64_t base = (uint64_t)qi * S;
  unsigned long long o = toff[(uint64_t)qi * ntiles + tile];
  for (uint32_t c = s0; c < s1; c += MK_ABV_THREADS) {
    const uint32_t s = c + t;
    const uint32_t f = s < s1 ? first[base + s] : MK_ABV_UNSET;
    const bool hit = f != MK_ABV_UNSET;
    const uint64_t b = __ballot(hit);
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if (lane == 0) wc[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < MK_ABV_THREADS / 64; w++) { if (w < wave) before += wc[w]; all += wc[w]; }
    if (hit) {
      const unsigned long long p = o + before + below;
      key[p] = f;
      val[p] = (uint32_t)p;
      ef[p] = f;
      em[p] = meas[base + s];
      es[p] = s;
      eq[p] = qi;
    }
    o += all;
    __syncthreads(); /* wc is rewritten by the next chunk */
  }
}

/* comparator_measure (:660-665) orders by a - b: -0 and +0 are equal; otherwise the float order (no NaN on this path) */
__global__ void __launch_bounds__(256) mk_abv_mkey_kernel(const uint32_t *val, uint64_t n, const float *em, uint32_t *key) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t b = __float_as_uint(em[val[i]]);
    if (b == 0x80000000u) b = 0u;
    key[i] = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  }
}

__global__ void __launch_bounds__(256) mk_abv_qkey_kernel(const uint32_t *val, uint64_t n, const uint32_t *eq, uint32_t *key) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) key[i] = eq[val[i]];
}

/* print order: ascending measure; cosine from the end (:329-331).  toff[q * ntiles] = the query's first output */
__global__ void __launch_bounds__(256) mk_abv_out_kernel(const uint32_t *val, uint64_t n, const uint32_t *eq, const uint32_t *es, const float *em,
                                                         const uint32_t *ef, const unsigned long long *toff, uint32_t ntiles, int reverse,
                                                         int32_t *os, float *om, uint32_t *of) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t p = val[i], qi = eq[p];
    uint64_t dst = i;
    if (reverse) dst = toff[(uint64_t)qi * ntiles] + toff[(uint64_t)(qi + 1) * ntiles] - 1 - i;
    os[dst] = (int32_t)es[p];
    om[dst] = em[p];
    of[dst] = ef[p];
  }
}

/* ---- host side ---------------------------------------------------------------------------------------- */

extern "C" int mk_abv_create(int device, mk_abv **out) {
  if (!out) return MK_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return mk_abv_fail(nullptr, MK_ERR_NO_DEVICE, "no HIP device: mk_abv has no CPU path");
  if (device < 0 || device >= ndev) return mk_abv_fail(nullptr, MK_ERR_NO_DEVICE, "device %d out of range (0..%d)", device, ndev - 1);
  mk_abv *a = new (std::nothrow) mk_abv();
  if (!a) return MK_ERR_NOMEM;
  a->device = device;
  hipDeviceProp_t prop;
  if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) {
    delete a;
    return mk_abv_fail(nullptr, MK_ERR_NO_DEVICE, "hipSetDevice(%d) failed", device);
  }
  a->num_cu = prop.multiProcessorCount;
  hipError_t r = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
  const size_t tmp_bytes = (size_t)256 * MK_RS_MAXB * 4 + 256 * 8 + 64;
  if (r == hipSuccess) r = mk_dev_alloc(&a->d_tmp, tmp_bytes);
  if (r == hipSuccess) r = mk_dev_alloc(&a->d_bad, 4);
  if (r == hipSuccess) r = mk_pin_alloc((void **)&a->h_sort_flag, 4 * sizeof(uint32_t), hipHostMallocDefault);
  if (r == hipSuccess) r = mk_pin_alloc((void **)&a->h_bad, 4, hipHostMallocDefault);
  for (int b = 0; b < 2 && r == hipSuccess; b++) {
    r = hipEventCreate(&a->ev_index[b]);
    if (r == hipSuccess) r = hipEventCreate(&a->ev_search[b]);
  }
  if (r != hipSuccess) {
    mk_abv_fail(nullptr, MK_ERR_NOMEM, "abv allocation: %s", hipGetErrorString(r));
    mk_abv_destroy(a);
    return MK_ERR_NOMEM;
  }
  *out = a;
  return MK_OK;
}

extern "C" int mk_abv_destroy(mk_abv *a) {
  if (!a) return MK_OK;
  (void)hipSetDevice(a->device);
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  void *dev[] = {a->d_in, a->d_key[0], a->d_key[1], a->d_val[0], a->d_val[1], a->d_tmp, a->d_fend, a->d_abm, a->d_abmi, a->d_ysum,
                 a->d_bad, a->d_col_s, a->d_col_p, a->d_lidx, a->d_yl2n, a->d_q, a->d_qoff, a->d_qnorm, a->d_nan, a->d_first,
                 a->d_meas, a->d_tcnt, a->d_toff, a->d_ef, a->d_es, a->d_eq, a->d_em, a->d_os, a->d_om, a->d_of};
  for (void *p : dev) (void)hipFree(p);
  void *pin[] = {a->h_sort_flag, a->h_bad, a->h_abm, a->h_abmi, a->h_yl2n, a->h_os, a->h_om, a->h_toff, a->h_nan};
  for (void *p : pin) if (p) (void)hipHostFree(p);
  for (int b = 0; b < 2; b++) {
    if (a->ev_index[b]) (void)hipEventDestroy(a->ev_index[b]);
    if (a->ev_search[b]) (void)hipEventDestroy(a->ev_search[b]);
  }
  if (a->stream) (void)hipStreamDestroy(a->stream);
  delete a;
  return MK_OK;
}

extern "C" const char *mk_abv_last_error(const mk_abv *a) { return a ? a->err : mk_abv_create_err; }

static int mk_abv_sort(mk_abv *a, uint32_t *key[2], uint32_t *val[2], uint64_t n, int *where) {
  uint32_t *hist = (uint32_t *)a->d_tmp;
  unsigned long long *tot = (unsigned long long *)((uint8_t *)a->d_tmp + (size_t)256 * MK_RS_MAXB * 4);
  uint32_t *flag = (uint32_t *)((uint8_t *)a->d_tmp + (size_t)256 * MK_RS_MAXB * 4 + 256 * 8);
  MK_ABV_HIP(a, mk_radix_sort_pairs_u32(key, val, n, a->num_cu, hist, tot, flag, a->h_sort_flag, a->stream, where));
  return MK_OK;
}

/* index_abv(), command_composite.c:347-440 */
extern "C" int mk_abv_index(mk_abv *a, const mk_binvec *entries, uint64_t n, const uint64_t *file_end, uint32_t nfiles, uint32_t nref,
                            const mk_binvec **abm, const int32_t **abmi, const double **yl2n, int64_t *bad_file) {
  if (!a || !abm || !abmi || !yl2n || (n && !entries) || (nfiles && !file_end)) return MK_ERR_ARG;
  if (bad_file) *bad_file = -1;
  if (n > 0x7FFFFFFFull) return mk_abv_fail(a, MK_ERR_ARG, "%llu entries: .abmi holds int32 counts (at most 2^31-1 entries)", (unsigned long long)n);
  if ((nfiles ? file_end[nfiles - 1] : 0) != n) return mk_abv_fail(a, MK_ERR_ARG, "file ends do not end at the entry count");
  for (uint32_t f = 1; f < nfiles; f++)
    if (file_end[f] < file_end[f - 1]) return mk_abv_fail(a, MK_ERR_ARG, "file ends not ascending at file %u", f);
  MK_ABV_HIP(a, hipSetDevice(a->device));
  int rc;
  if ((rc = mk_abv_grow_pinned(a, &a->h_abm, &a->h_abm_cap, n)) || (rc = mk_abv_grow_pinned(a, &a->h_abmi, &a->h_abmi_cap, nref)) ||
      (rc = mk_abv_grow_pinned(a, &a->h_yl2n, &a->h_yl2n_cap, nfiles)))
    return rc;
  if ((rc = mk_abv_grow(a, &a->d_in, &a->in_cap, n)) || (rc = mk_abv_grow(a, &a->d_fend, &a->fend_cap, nfiles)) ||
      (rc = mk_abv_grow(a, &a->d_abm, &a->abm_cap, n)) || (rc = mk_abv_grow(a, &a->d_abmi, &a->abmi_cap, nref)) ||
      (rc = mk_abv_grow(a, &a->d_ysum, &a->ysum_cap, nfiles)))
    return rc;
  for (int b = 0; b < 2; b++)
    if ((rc = mk_abv_grow(a, &a->d_key[b], &a->pair_cap[b], n)) || (rc = mk_abv_grow(a, &a->d_val[b], &a->pair_cap[2 + b], n))) return rc;
  if (n) MK_ABV_HIP(a, hipMemcpyAsync(a->d_in, entries, n * sizeof(mk_binvec), hipMemcpyHostToDevice, a->stream));
  if (nfiles) MK_ABV_HIP(a, hipMemcpyAsync(a->d_fend, file_end, (size_t)nfiles * 8, hipMemcpyHostToDevice, a->stream));
  MK_ABV_HIP(a, hipMemsetAsync(a->d_bad, 0xFF, 4, a->stream));
  a->index_timed = false;
  MK_ABV_HIP(a, hipEventRecord(a->ev_index[0], a->stream));
  if (n) {
    hipLaunchKernelGGL(mk_abv_prep_kernel, dim3(mk_abv_blocks(a, n, 256)), dim3(256), 0, a->stream, (const mk_binvec *)a->d_in, n, nref,
                       a->d_key[0], a->d_val[0], a->d_bad);
    MK_ABV_HIP(a, hipGetLastError());
    MK_ABV_HIP(a, hipMemcpyAsync(a->h_bad, a->d_bad, 4, hipMemcpyDeviceToHost, a->stream));
    MK_ABV_HIP(a, hipStreamSynchronize(a->stream));
    if (*a->h_bad != 0xFFFFFFFFu) {
      const uint64_t p = *a->h_bad;
      const uint32_t f = (uint32_t)(std::upper_bound(file_end, file_end + nfiles, p) - file_end);
      if (bad_file) *bad_file = f;
      return mk_abv_fail(a, MK_ERR_FORMAT, "file %u entry %llu: species %d outside 0..%u", f, (unsigned long long)(p - (f ? file_end[f - 1] : 0)),
                         entries[p].ref_idx, nref ? nref - 1 : 0);
    }
  }
  int where = 0;
  if ((rc = mk_abv_sort(a, a->d_key, a->d_val, n, &where))) return rc;
  if (n)
    hipLaunchKernelGGL(mk_abv_gather_kernel, dim3(mk_abv_blocks(a, n, 256)), dim3(256), 0, a->stream, (const mk_binvec *)a->d_in,
                       (const uint32_t *)a->d_val[where], n, (const unsigned long long *)a->d_fend, nfiles, a->d_abm);
  if (nref)
    hipLaunchKernelGGL(mk_abv_abmi_kernel, dim3(mk_abv_blocks(a, nref, 256)), dim3(256), 0, a->stream, (const uint32_t *)a->d_key[where], n,
                       nref, a->d_abmi);
  if (nfiles)
    hipLaunchKernelGGL(mk_abv_yl2n_kernel, dim3(mk_abv_blocks(a, nfiles, 256)), dim3(256), 0, a->stream, (const mk_binvec *)a->d_in,
                       (const unsigned long long *)a->d_fend, nfiles, a->d_ysum);
  MK_ABV_HIP(a, hipGetLastError());
  MK_ABV_HIP(a, hipEventRecord(a->ev_index[1], a->stream));
  a->index_timed = true;
  if (n) MK_ABV_HIP(a, hipMemcpyAsync(a->h_abm, a->d_abm, n * sizeof(mk_binvec), hipMemcpyDeviceToHost, a->stream));
  if (nref) MK_ABV_HIP(a, hipMemcpyAsync(a->h_abmi, a->d_abmi, (size_t)nref * 4, hipMemcpyDeviceToHost, a->stream));
  if (nfiles) MK_ABV_HIP(a, hipMemcpyAsync(a->h_yl2n, a->d_ysum, (size_t)nfiles * 8, hipMemcpyDeviceToHost, a->stream));
  MK_ABV_HIP(a, hipStreamSynchronize(a->stream));
  for (uint32_t f = 0; f < nfiles; f++) a->h_yl2n[f] = std::sqrt(a->h_yl2n[f]); /* :402 (libm's sqrt, correctly rounded) */
  *abm = a->h_abm;
  *abmi = a->h_abmi;
  *yl2n = a->h_yl2n;
  return MK_OK;
}

/* abv_search() :214-252: the index files, resident on the device until the next load / destroy */
extern "C" int mk_abv_load(mk_abv *a, const mk_binvec *abm, uint64_t n, const int32_t *abmi, uint32_t nref, const double *yl2n,
                           uint32_t nsamples) {
  if (!a || (n && !abm) || (nref && !abmi) || (nsamples && !yl2n)) return MK_ERR_ARG;
  a->loaded = false;
  if (n > 0xFFFFFFFFull) return mk_abv_fail(a, MK_ERR_ARG, "index of %llu entries", (unsigned long long)n);
  for (uint32_t r = 0; r < nref; r++) /* the columns must lie inside the matrix */
    if (abmi[r] < (r ? abmi[r - 1] : 0) || (uint64_t)abmi[r] > n)
      return mk_abv_fail(a, MK_ERR_FORMAT, ".abmi not ascending inside 0..%llu at species %u", (unsigned long long)n, r);
  MK_ABV_HIP(a, hipSetDevice(a->device));
  int rc;
  if ((rc = mk_abv_grow(a, &a->d_in, &a->in_cap, n)) || (rc = mk_abv_grow(a, &a->d_col_s, &a->col_cap[0], n)) ||
      (rc = mk_abv_grow(a, &a->d_col_p, &a->col_cap[1], n)) || (rc = mk_abv_grow(a, &a->d_lidx, &a->lidx_cap, nref)) ||
      (rc = mk_abv_grow(a, &a->d_yl2n, &a->yl2n_cap, nsamples)))
    return rc;
  if (n) MK_ABV_HIP(a, hipMemcpyAsync(a->d_in, abm, n * sizeof(mk_binvec), hipMemcpyHostToDevice, a->stream));
  if (nref) MK_ABV_HIP(a, hipMemcpyAsync(a->d_lidx, abmi, (size_t)nref * 4, hipMemcpyHostToDevice, a->stream));
  if (nsamples) MK_ABV_HIP(a, hipMemcpyAsync(a->d_yl2n, yl2n, (size_t)nsamples * 8, hipMemcpyHostToDevice, a->stream));
  MK_ABV_HIP(a, hipMemsetAsync(a->d_bad, 0xFF, 4, a->stream));
  if (n)
    hipLaunchKernelGGL(mk_abv_split_kernel, dim3(mk_abv_blocks(a, n, 256)), dim3(256), 0, a->stream, (const mk_binvec *)a->d_in, n, a->d_col_s,
                       a->d_col_p);
  if (nref)
    hipLaunchKernelGGL(mk_abv_check_kernel, dim3(mk_abv_blocks(a, nref, 256)), dim3(256), 0, a->stream, (const uint32_t *)a->d_col_s,
                       (const int32_t *)a->d_lidx, nref, nsamples, a->d_bad);
  MK_ABV_HIP(a, hipGetLastError());
  MK_ABV_HIP(a, hipMemcpyAsync(a->h_bad, a->d_bad, 4, hipMemcpyDeviceToHost, a->stream));
  MK_ABV_HIP(a, hipStreamSynchronize(a->stream));
  if (*a->h_bad != 0xFFFFFFFFu)
    return mk_abv_fail(a, MK_ERR_FORMAT, "species %u: its column names a sample outside 0..%u or does not ascend (not an index made by -i)",
                       *a->h_bad, nsamples ? nsamples - 1 : 0);
  a->n = n;
  a->nref = nref;
  a->nsamples = nsamples;
  a->loaded = true;
  return MK_OK;
}

/* glibc 2.35 msort_with_tmp (qsort of abv_search, :304/:309/:314) with comparator_measure: exact even where a NaN makes the
 * comparator inconsistent */
static int mk_abv_cmp(const float *m, uint32_t i, uint32_t j) {
  const float r = m[i] - m[j];
  if (r > 0) return 1;
  if (r < 0) return -1;
  return 0;
}
static void mk_abv_msort(uint32_t *b, uint64_t n, uint32_t *tmp, const float *m) {
  if (n <= 1) return;
  uint64_t n1 = n / 2, n2 = n - n1;
  uint32_t *b1 = b, *b2 = b + n1, *t = tmp;
  mk_abv_msort(b1, n1, tmp, m);
  mk_abv_msort(b2, n2, tmp, m);
  while (n1 > 0 && n2 > 0) {
    if (mk_abv_cmp(m, *b1, *b2) <= 0) { *t++ = *b1++; n1--; }
    else { *t++ = *b2++; n2--; }
  }
  if (n1 > 0) memcpy(t, b1, n1 * 4);
  memcpy(b, tmp, (n - n2) * 4);
}

/* abv_search() :254-335 for nq query vectors (entries concatenated, q_end cumulative) */
extern "C" int mk_abv_search(mk_abv *a, int metric, uint32_t nq, const mk_binvec *q, const uint64_t *q_end, uint64_t *out_end,
                             const int32_t **samples, const float **measures, int64_t *bad_query) {
  if (!a || !out_end || !samples || !measures || (nq && !q_end)) return MK_ERR_ARG;
  if (bad_query) *bad_query = -1;
  if (metric < 0 || metric > 2) return mk_abv_fail(a, MK_ERR_ARG, "metric %d: 0 cosine, 1 L1, 2 L2", metric);
  if (!a->loaded) return mk_abv_fail(a, MK_ERR_STATE, "mk_abv_search before mk_abv_load");
  const uint64_t nd = nq ? q_end[nq - 1] : 0;
  if (nd && !q) return MK_ERR_ARG;
  const uint32_t S = a->nsamples, ntiles = (S + MK_ABV_TILE - 1) / MK_ABV_TILE;
  if ((uint64_t)nq * S > 0xFFFFFFFFull) return mk_abv_fail(a, MK_ERR_ARG, "%u queries x %u samples: search fewer queries per call", nq, S);
  /* the query's own norm, :258/:289: a float sum in file order; the species must name a column (the reference reads past .abmi) */
  std::vector<unsigned long long> qoff((size_t)nq + 1, 0);
  std::vector<double> qnorm(nq ? nq : 1);
  for (uint32_t k = 0; k < nq; k++) {
    const uint64_t lo = k ? q_end[k - 1] : 0, hi = q_end[k];
    if (hi < lo) return mk_abv_fail(a, MK_ERR_ARG, "query ends not ascending at query %u", k);
    float xl2n = 0;
    for (uint64_t d = lo; d < hi; d++) {
      if (q[d].ref_idx < 0 || (uint32_t)q[d].ref_idx >= a->nref) {
        if (bad_query) *bad_query = k;
        return mk_abv_fail(a, MK_ERR_FORMAT, "query %u entry %llu: species %d outside 0..%d of the index", k, (unsigned long long)(d - lo),
                           q[d].ref_idx, (int)a->nref - 1);
      }
      const float pp = q[d].pct * q[d].pct;
      xl2n = xl2n + pp;
    }
    qnorm[k] = std::sqrt((double)xl2n);
    qoff[k + 1] = hi;
  }
  MK_ABV_HIP(a, hipSetDevice(a->device));
  int rc;
  const uint64_t dense = (uint64_t)nq * S, nt = (uint64_t)nq * ntiles;
  if ((rc = mk_abv_grow(a, &a->d_q, &a->q_cap, nd)) || (rc = mk_abv_grow(a, &a->d_qoff, &a->qn_cap[0], (uint64_t)nq + 1)) ||
      (rc = mk_abv_grow(a, &a->d_qnorm, &a->qn_cap[1], nq)) || (rc = mk_abv_grow(a, &a->d_nan, &a->qn_cap[2], nq)))
    return rc;
  if ((rc = mk_abv_grow(a, &a->d_first, &a->dense_cap[0], dense)) || (rc = mk_abv_grow(a, &a->d_meas, &a->dense_cap[1], dense)) ||
      (rc = mk_abv_grow(a, &a->d_tcnt, &a->t_cap[0], nt)) || (rc = mk_abv_grow(a, &a->d_toff, &a->t_cap[1], nt + 1)) ||
      (rc = mk_abv_grow_pinned(a, &a->h_toff, &a->h_toff_cap, nt + 1)) || (rc = mk_abv_grow_pinned(a, &a->h_nan, &a->h_nan_cap, nq)))
    return rc;
  if (nd) MK_ABV_HIP(a, hipMemcpyAsync(a->d_q, q, nd * sizeof(mk_binvec), hipMemcpyHostToDevice, a->stream));
  MK_ABV_HIP(a, hipMemcpyAsync(a->d_qoff, qoff.data(), ((size_t)nq + 1) * 8, hipMemcpyHostToDevice, a->stream));
  if (nq) MK_ABV_HIP(a, hipMemcpyAsync(a->d_qnorm, qnorm.data(), (size_t)nq * 8, hipMemcpyHostToDevice, a->stream));
  MK_ABV_HIP(a, hipMemsetAsync(a->d_nan, 0, (size_t)(nq ? nq : 1) * 4, a->stream));
  a->search_timed = false;
  MK_ABV_HIP(a, hipEventRecord(a->ev_search[0], a->stream));
  if (nq && ntiles) {
    const dim3 grid(ntiles, nq);
    const uint32_t *cs = a->d_col_s;
    const float *cp = a->d_col_p;
    const int32_t *ci = a->d_lidx;
    const double *yl = a->d_yl2n, *qn = a->d_qnorm;
    const unsigned long long *qo = a->d_qoff;
    const mk_binvec *qq = a->d_q;
    if (metric == 1)
      hipLaunchKernelGGL(mk_abv_search_kernel<1>, grid, dim3(MK_ABV_THREADS), 0, a->stream, cs, cp, ci, yl, S, ntiles, qq, qo, qn, a->d_first, a->d_meas, a->d_tcnt, a->d_nan);
    else if (metric == 2)
      hipLaunchKernelGGL(mk_abv_search_kernel<2>, grid, dim3(MK_ABV_THREADS), 0, a->stream, cs, cp, ci, yl, S, ntiles, qq, qo, qn, a->d_first, a->d_meas, a->d_tcnt, a->d_nan);
    else
      hipLaunchKernelGGL(mk_abv_search_kernel<0>, grid, dim3(MK_ABV_THREADS), 0, a->stream, cs, cp, ci, yl, S, ntiles, qq, qo, qn, a->d_first, a->d_meas, a->d_tcnt, a->d_nan);
    MK_ABV_HIP(a, hipGetLastError());
    hipLaunchKernelGGL(mk_abv_scan_kernel, dim3(1), dim3(1024), 0, a->stream, (const uint32_t *)a->d_tcnt, nt, a->d_toff);
    MK_ABV_HIP(a, hipGetLastError());
  } else {
    MK_ABV_HIP(a, hipMemsetAsync(a->d_toff, 0, (nt + 1) * 8, a->stream));
  }
  MK_ABV_HIP(a, hipMemcpyAsync(a->h_toff, a->d_toff, (nt + 1) * 8, hipMemcpyDeviceToHost, a->stream));
  if (nq) MK_ABV_HIP(a, hipMemcpyAsync(a->h_nan, a->d_nan, (size_t)nq * 4, hipMemcpyDeviceToHost, a->stream));
  MK_ABV_HIP(a, hipStreamSynchronize(a->stream));
  const uint64_t M = a->h_toff[nt];
  if ((rc = mk_abv_grow_pinned(a, &a->h_os, &a->h_o_cap[0], M)) || (rc = mk_abv_grow_pinned(a, &a->h_om, &a->h_o_cap[1], M))) return rc;
  if (M) {
    for (int b = 0; b < 2; b++)
      if ((rc = mk_abv_grow(a, &a->d_key[b], &a->pair_cap[b], M)) || (rc = mk_abv_grow(a, &a->d_val[b], &a->pair_cap[2 + b], M))) return rc;
    if ((rc = mk_abv_grow(a, &a->d_ef, &a->e_cap[0], M)) || (rc = mk_abv_grow(a, &a->d_es, &a->e_cap[1], M)) ||
        (rc = mk_abv_grow(a, &a->d_eq, &a->e_cap[2], M)) || (rc = mk_abv_grow(a, &a->d_em, &a->e_cap[3], M)) ||
        (rc = mk_abv_grow(a, &a->d_os, &a->o_cap[0], M)) || (rc = mk_abv_grow(a, &a->d_om, &a->o_cap[1], M)) ||
        (rc = mk_abv_grow(a, &a->d_of, &a->o_cap[2], M)))
      return rc;
    hipLaunchKernelGGL(mk_abv_emit_kernel, dim3(ntiles, nq), dim3(MK_ABV_THREADS), 0, a->stream, (const uint32_t *)a->d_first,
                       (const float *)a->d_meas, S, ntiles, (const unsigned long long *)a->d_toff, a->d_key[0], a->d_val[0], a->d_ef, a->d_em,
                       a->d_es, a->d_eq);
    MK_ABV_HIP(a, hipGetLastError());
    /* LSD over (query, measure, first entry, sample): the emit order is (query, sample) */
    int w = 0;
    if ((rc = mk_abv_sort(a, a->d_key, a->d_val, M, &w))) return rc;
    uint32_t *k2[2] = {a->d_key[w], a->d_key[w ^ 1]}, *v2[2] = {a->d_val[w], a->d_val[w ^ 1]};
    hipLaunchKernelGGL(mk_abv_mkey_kernel, dim3(mk_abv_blocks(a, M, 256)), dim3(256), 0, a->stream, (const uint32_t *)v2[0], M,
                       (const float *)a->d_em, k2[0]);
    MK_ABV_HIP(a, hipGetLastError());
    int w2 = 0;
    if ((rc = mk_abv_sort(a, k2, v2, M, &w2))) return rc;
    uint32_t *k3[2] = {k2[w2], k2[w2 ^ 1]}, *v3[2] = {v2[w2], v2[w2 ^ 1]};
    hipLaunchKernelGGL(mk_abv_qkey_kernel, dim3(mk_abv_blocks(a, M, 256)), dim3(256), 0, a->stream, (const uint32_t *)v3[0], M,
                       (const uint32_t *)a->d_eq, k3[0]);
    MK_ABV_HIP(a, hipGetLastError());
    int w3 = 0;
    if ((rc = mk_abv_sort(a, k3, v3, M, &w3))) return rc;
    hipLaunchKernelGGL(mk_abv_out_kernel, dim3(mk_abv_blocks(a, M, 256)), dim3(256), 0, a->stream, (const uint32_t *)v3[w3], M,
                       (const uint32_t *)a->d_eq, (const uint32_t *)a->d_es, (const float *)a->d_em, (const uint32_t *)a->d_ef,
                       (const unsigned long long *)a->d_toff, ntiles, metric == 0 ? 1 : 0, a->d_os, a->d_om, a->d_of);
    MK_ABV_HIP(a, hipGetLastError());
  }
  MK_ABV_HIP(a, hipEventRecord(a->ev_search[1], a->stream));
  a->search_timed = true;
  if (M) {
    MK_ABV_HIP(a, hipMemcpyAsync(a->h_os, a->d_os, M * 4, hipMemcpyDeviceToHost, a->stream));
    MK_ABV_HIP(a, hipMemcpyAsync(a->h_om, a->d_om, M * 4, hipMemcpyDeviceToHost, a->stream));
  }
  MK_ABV_HIP(a, hipStreamSynchronize(a->stream));
  for (uint32_t k = 0; k < nq; k++) out_end[k] = a->h_toff[(uint64_t)(k + 1) * ntiles];
  /* a query with a NaN measure: discovery order from (first entry, sample), then glibc's merge sort as it runs */
  for (uint32_t k = 0; k < nq; k++) {
    if (!a->h_nan[k]) continue;
    const uint64_t lo = k ? out_end[k - 1] : 0, cnt = out_end[k] - lo;
    std::vector<uint32_t> f(cnt);
    MK_ABV_HIP(a, hipMemcpy(f.data(), a->d_of + lo, cnt * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> ord(cnt), tmp(cnt);
    for (uint64_t i = 0; i < cnt; i++) ord[i] = (uint32_t)i;
    const int32_t *s = a->h_os + lo;
    std::sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return f[x] != f[y] ? f[x] < f[y] : s[x] < s[y]; });
    std::vector<float> mv(a->h_om + lo, a->h_om + lo + cnt);
    std::vector<int32_t> sv(s, s + cnt);
    mk_abv_msort(ord.data(), cnt, tmp.data(), mv.data());
    for (uint64_t i = 0; i < cnt; i++) {
      const uint64_t dst = metric == 0 ? cnt - 1 - i : i;
      a->h_os[lo + dst] = sv[ord[i]];
      a->h_om[lo + dst] = mv[ord[i]];
    }
  }
  *samples = a->h_os;
  *measures = a->h_om;
  return MK_OK;
}

/* measurement: device time of the last mk_abv_index's kernels (prep, sort, gather, abmi, yl2n) and of the last mk_abv_search's
 * (accumulation, compaction, the three sorts, output order), from HIP events on the handle's stream; 0 for what has not run */
extern "C" int mk_abv_last_kernel_ms(mk_abv *a, double *index_ms, double *search_ms) {
  if (!a || !index_ms || !search_ms) return MK_ERR_ARG;
  *index_ms = *search_ms = 0.0;
  MK_ABV_HIP(a, hipSetDevice(a->device));
  float f = 0.f;
  if (a->index_timed) { MK_ABV_HIP(a, hipEventSynchronize(a->ev_index[1])); MK_ABV_HIP(a, hipEventElapsedTime(&f, a->ev_index[0], a->ev_index[1])); *index_ms = (double)f; }
  if (a->search_timed) { MK_ABV_HIP(a, hipEventSynchronize(a->ev_search[1])); MK_ABV_HIP(a, hipEventElapsedTime(&f, a->ev_search[0], a->ev_search[1])); *search_ms = (double)f; }
  return MK_OK;
}
