/*
 * mk_byread.hip -- `dist --byread` and `reverse` on the device (gfx950, wave64, hand-written).
 *
 * reads2mco() (iseq2comem.c:88-214) walks a file byte by byte exactly like fasta2co() and, for every full window whose canonical
 * k-mer passes the .shuf test, APPENDS drtuple >> comp_code_bits to the file of component drtuple % component_num and counts it
 * for the record (number of '>' seen so far) it lies in: no hash table, no deduplication, key 0 kept, repeats kept, text order.
 * Behind the walk it writes, per component, the cumulative counts over the records.  That is an ordered compaction:
 *
 *   mk_fa_summary_kernel / mk_fa_emit_kernel (mk_stream.hip.h)  text -> base stream; a header line leaves its '>' as ONE byte
 *   mk_br_fa_scan_kernel   composes the segment summaries (mk_fa_compose) from the header state carried between pushes
 *   mk_br_count_kernel     a wave per chunk of 1024 stream positions: the window ending at each position from LDS, mk_accept_key
 *                          (mk_key.hip.h: the resolve kernel's test and key), accepted windows per component and '>' bytes per chunk
 *   mk_br_scan_kernel      one workgroup per component (+ one for '>'): exclusive prefix over the chunks, totals
 *   mk_br_write_kernel     the same walk again with every chunk's offsets known: ids to their component's block in stream order
 *                          (ballot ranks: a stable split), beside each id the number of '>' in front of it = its record in this push
 *   mk_br_index_kernel     per (component, record of this push): ids of the component with a record number <= it (binary search in
 *                          the ascending record numbers) + the component's count before this push = the entry of combco.index.<c>
 *   mk_br_carry_kernel     the last TL-1 stream bytes move to the front of the stream buffer: the next push's first windows
 * Positions, counts and record numbers of a file are 64-bit (host side and index entries); inside one push (at most
 * MK_BYREAD_MAX_PUSH bytes) they are 32-bit offsets.  Nothing depends on the length of a record.
 *
 * co_reverse2kmer() / co_rvs2kmer_byreads() (command_reverse.c:148-368) turn an id back into its canonical k-mer through
 * core_reverse2unituple() (:355-368) and print it with one fprintf per k-mer:
 *   mk_br_reverse_kernel   256 ids per workgroup: each thread inverts one id and lays its line of 2k letters + '\n' into LDS; the
 *                          workgroup then stores the 256 lines as 16-byte vectors (256 * (2k+1) bytes is a multiple of 16)
 * Bound of every kernel here: HBM traffic (DESIGN.md 4.9 has the bytes per kernel and the measured times).
 */
#include <hip/hip_runtime.h>
#include "mk_poison.hip.h"

namespace { /* mk_engine.hip holds the stream kernels too: this file's copies stay local */
#include "mk_key.hip.h"
#include "mk_stream.hip.h"
}

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "metakssd_hip.h"

#define MK_BR_CHUNK 1024u /* stream positions per wave */
#define MK_BR_WAVES 4u
#define MK_BR_MAXC 16u    /* component_num is 1 or 16 (mk_params_init) */
#define MK_BR_ROWS (MK_BR_MAXC + 1u) /* chunk-count rows: one per component, the last for '>' */
#define MK_BR_REV_IDS 256u
#define MK_BR_REV_BATCH (1u << 22) /* ids per reverse launch: at most 132 MiB of text on the device */

namespace {

struct mk_br_state {
  unsigned long long kept; /* stream bytes the last push added behind the TL-1 carried ones */
  uint32_t in_header;      /* state behind the text pushed so far */
  uint32_t pad;
  unsigned long long totals[MK_BR_ROWS]; /* last push: ids per component, '>' bytes */
};

struct mk_br_args {
  const uint8_t *stream; /* [TL-1 carried bytes][kept new bytes] */
  const mk_br_state *st;
  mk_keyparams kp;
  const uint32_t *accept_bits;
  const int32_t *shuf;
  uint32_t comp_num, comp_code_bits, nchunks;
};

__global__ void __launch_bounds__(1024) mk_br_fa_scan_kernel(mk_fa_sum *sum, uint64_t nseg, mk_br_state *st) {
  unsigned long long kept;
  uint32_t state;
  mk_fa_compose(sum, nseg, st->in_header, kept, state);
  __syncthreads(); /* (every thread has read st->in_header before thread 0 writes it) */
  if (threadIdx.x == 0) { st->kept = kept; st->in_header = state; }
}

/* accept_bits of a whole .shuf table (the engine builds its own from the accepted pairs; here the table is on the device) */
__global__ void __launch_bounds__(256) mk_br_accept_kernel(const int32_t *shuf, uint64_t len, int32_t dim_start, int32_t dim_end, uint32_t *bits) {
  const uint64_t words = (len + 31u) / 32u;
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t m = 0;
    for (uint32_t b = 0; b < 32u; b++) {
      const uint64_t d = w * 32u + b;
      if (d < len) { const int32_t pf = shuf[d]; if (pf >= dim_start && pf < dim_end) m |= 1u << b; }
    }
    bits[w] = m;
  }
}

/* the wave's chunk of the stream, positions [c0, c0 + MK_BR_CHUNK) with their TL-1 bytes in front, into the wave's LDS.  The
 * window that ENDS at new byte i is stream[i .. i + TL - 1]; bytes behind the stream's end are never looked at (the walk masks
 * their positions; the buffer ends in slack, so the loads themselves may run past it) */
__device__ __forceinline__ const uint8_t *mk_br_stage(const uint8_t *stream, uint64_t c0, uint32_t lane, uint4 *lds) {
  lds[lane] = *(const uint4 *)(stream + c0 + 16u * lane);
  if (lane < 2u) lds[64u + lane] = *(const uint4 *)(stream + c0 + MK_BR_CHUNK + 16u * lane);
  mk_wave_lds_fence();
  return (const uint8_t *)lds;
}

/* the window of TL bytes at `win`: false unless all of them are bases and the canonical k-mer is accepted (iseq2comem.c:136-194) */
__device__ __forceinline__ bool mk_br_window(const mk_br_args &a, const uint8_t *win, uint64_t &drtuple) {
  uint64_t fwd = 0;
  bool ok = true;
  for (uint32_t j = 0; j < a.kp.TL; j++) {
    const uint32_t ch = win[j], u = ch | 0x20u;
    ok = ok && (u == 'a' || u == 'c' || u == 'g' || u == 't');
    const uint32_t c = (ch >> 1) & 3u; /* A=0 C=1 T=2 G=3 */
    fwd = (fwd << 2) | (uint64_t)(c ^ (c >> 1)); /* the reference's A=0 C=1 G=2 T=3 (Basemap, global_basic.c:62-69) */
  }
  if (!ok) return false;
  const uint64_t rc = mk_revcomp(fwd, a.kp.TL);
  return mk_accept_key(a.kp, a.accept_bits, a.shuf, fwd < rc ? fwd : rc, drtuple);
}

/* chunk_count is [MK_BR_ROWS][nchunks]; every entry of the rows in use is written (chunks behind the stream's end: 0) */
__global__ void __launch_bounds__(64 * MK_BR_WAVES) mk_br_count_kernel(mk_br_args a, uint32_t *chunk_count) {
  __shared__ uint4 lds[MK_BR_WAVES][66];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t chunk = blockIdx.x * MK_BR_WAVES + wave;
  if (chunk >= a.nchunks) return;
  const unsigned long long kept = a.st->kept;
  const uint64_t c0 = (uint64_t)chunk * MK_BR_CHUNK;
  uint32_t mine = 0, gts = 0; /* lane c (< comp_num) accumulates component c */
  if (c0 < kept) {
    const uint8_t *seg = mk_br_stage(a.stream, c0, lane, lds[wave]);
    for (uint32_t it = 0; it < MK_BR_CHUNK / 64u; it++) {
      if (c0 + 64u * it >= kept) break;
      const bool valid = c0 + 64u * it + lane < kept;
      const uint8_t *win = seg + 64u * it + lane;
      gts += (uint32_t)__popcll(__ballot(valid && win[a.kp.TL - 1u] == '>'));
      uint64_t dr = 0;
      const bool p = valid && mk_br_window(a, win, dr);
      const uint32_t comp = (uint32_t)(dr % a.comp_num);
      uint64_t rest = __ballot(p);
      while (rest) { /* one round per distinct component present among the 64 positions */
        const uint32_t c = __shfl(comp, (int)__builtin_ctzll(rest));
        const uint64_t m = __ballot(p && comp == c);
        if (lane == c) mine += (uint32_t)__popcll(m);
        rest &= ~m;
      }
    }
  }
  if (lane < a.comp_num) chunk_count[(size_t)lane * a.nchunks + chunk] = mine;
  if (lane == 0) chunk_count[(size_t)MK_BR_MAXC * a.nchunks + chunk] = gts;
}

/* workgroup r < comp_num: component r; workgroup comp_num: the '>' row.  Exclusive scan of the row in place, its total to st */
__global__ void __launch_bounds__(1024) mk_br_scan_kernel(uint32_t *chunk_count, uint32_t nchunks, uint32_t comp_num, mk_br_state *st) {
  __shared__ unsigned long long wsum[16];
  __shared__ unsigned long long carry_s;
  const uint32_t row = blockIdx.x < comp_num ? blockIdx.x : MK_BR_MAXC;
  uint32_t *cc = chunk_count + (size_t)row * nchunks;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (uint32_t base = 0; base < nchunks; base += 1024u) {
    const uint32_t i = base + threadIdx.x;
    unsigned long long v = i < nchunks ? cc[i] : 0ull, incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      unsigned long long t = __shfl_up(incl, o);
      if ((int)lane >= o) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned long long woff = 0;
    for (uint32_t w = 0; w < wave; w++) woff += wsum[w];
    const unsigned long long carry = carry_s;
    if (i < nchunks) cc[i] = (uint32_t)(carry + woff + incl - v);
    __syncthreads();
    if (threadIdx.x == 1023) carry_s = carry + woff + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) st->totals[row] = carry_s;
}

/* ids / rec hold the components back to back: component c starts at sum(totals[0..c)) */
__global__ void __launch_bounds__(64 * MK_BR_WAVES) mk_br_write_kernel(mk_br_args a, const uint32_t *chunk_off, uint32_t *ids, uint32_t *rec) {
  __shared__ uint4 lds[MK_BR_WAVES][66];
  __shared__ uint32_t wbase[MK_BR_WAVES][MK_BR_MAXC];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t chunk = blockIdx.x * MK_BR_WAVES + wave;
  if (chunk >= a.nchunks) return;
  const unsigned long long kept = a.st->kept;
  const uint64_t c0 = (uint64_t)chunk * MK_BR_CHUNK;
  if (c0 >= kept) return;
  if (lane < a.comp_num) {
    unsigned long long start = 0;
    for (uint32_t c = 0; c < lane; c++) start += a.st->totals[c];
    wbase[wave][lane] = (uint32_t)start + chunk_off[(size_t)lane * a.nchunks + chunk];
  }
  uint32_t gtbase = chunk_off[(size_t)MK_BR_MAXC * a.nchunks + chunk]; /* '>' bytes of this push in front of the chunk */
  const uint8_t *seg = mk_br_stage(a.stream, c0, lane, lds[wave]); /* (its fence orders wbase too) */
  for (uint32_t it = 0; it < MK_BR_CHUNK / 64u; it++) {
    if (c0 + 64u * it >= kept) break;
    const bool valid = c0 + 64u * it + lane < kept;
    const uint8_t *win = seg + 64u * it + lane;
    const uint64_t gt = __ballot(valid && win[a.kp.TL - 1u] == '>');
    const uint32_t myrec = gtbase + mk_mbcnt(gt); /* '>' in front of this position (an emitting position is a base itself) */
    gtbase += (uint32_t)__popcll(gt);
    uint64_t dr = 0;
    const bool p = valid && mk_br_window(a, win, dr);
    const uint32_t comp = (uint32_t)(dr % a.comp_num);
    uint64_t rest = __ballot(p);
    while (rest) {
      const uint32_t c = __shfl(comp, (int)__builtin_ctzll(rest));
      const bool sel = p && comp == c;
      const uint64_t m = __ballot(sel);
      const uint32_t base = wbase[wave][c];
      if (sel) {
        const uint32_t o = base + mk_mbcnt(m);
        ids[o] = (uint32_t)(dr >> a.comp_code_bits);
        rec[o] = myrec;
      }
      mk_wave_lds_fence();
      if (lane == 0) wbase[wave][c] = base + (uint32_t)__popcll(m);
      mk_wave_lds_fence();
      rest &= ~m;
    }
  }
}

struct mk_br_index_args {
  unsigned long long before[MK_BR_MAXC]; /* ids of the component in front of this push */
  uint32_t start[MK_BR_MAXC + 1u];       /* the component's block in ids / rec */
};
/* out[c * nrec + j] = before[c] + (ids of component c in this push whose record is <= j): rec ascends inside a block */
__global__ void __launch_bounds__(256) mk_br_index_kernel(mk_br_index_args x, const uint32_t *rec, uint32_t comp_num, uint64_t nrec,
                                                          unsigned long long *out) {
  const uint64_t n = (uint64_t)comp_num * nrec;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t c = (uint32_t)(e / nrec);
    const uint64_t j = e - (uint64_t)c * nrec;
    uint32_t lo = x.start[c], hi = x.start[c + 1u];
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if ((uint64_t)rec[mid] <= j) lo = mid + 1u; else hi = mid;
    }
    out[e] = x.before[c] + (lo - x.start[c]);
  }
}

/* one wave: every lane reads before any lane writes, so the ranges may overlap (a push that kept fewer than TL-1 bytes) */
__global__ void __launch_bounds__(64) mk_br_carry_kernel(uint8_t *stream, const mk_br_state *st, uint32_t ncarry) {
  const uint32_t lane = threadIdx.x;
  uint8_t b = 0;
  if (lane < ncarry) b = stream[st->kept + lane];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane < ncarry) stream[lane] = b;
}

__global__ void __launch_bounds__(64) mk_br_reset_kernel(uint8_t *stream, mk_br_state *st, uint32_t ncarry) {
  const uint32_t lane = threadIdx.x;
  if (lane < ncarry) stream[lane] = (uint8_t)'N'; /* no base: no window reaches in front of the file */
  if (lane == 0) { st->kept = 0ull; st->in_header = 0u; st->pad = 0u; }
  if (lane < MK_BR_ROWS) st->totals[lane] = 0ull;
}

struct mk_br_rev_args {
  const uint32_t *ids;
  uint64_t n;
  const uint32_t *rev; /* rev_shuf_arr[4096], command_reverse.c:152-160 */
  uint32_t comp, comp_code_bits, pf_bits, inner_bits, hob /*half_outer_ctx_bits*/, TL;
};
/* core_reverse2unituple() (command_reverse.c:355-368) + the letter loop (:344-348).  out: lines of TL + 1 bytes; the buffer is
 * padded to whole workgroups, so every store is a full 16-byte vector */
__global__ void __launch_bounds__(MK_BR_REV_IDS) mk_br_reverse_kernel(mk_br_rev_args a, uint4 *out) {
  __shared__ uint4 lines4[MK_BR_REV_IDS * 33u / 16u]; /* 256 lines of at most 33 bytes */
  uint8_t *lines = (uint8_t *)lines4;
  const uint32_t W = a.TL + 1u;
  const uint64_t i = (uint64_t)blockIdx.x * MK_BR_REV_IDS + threadIdx.x;
  if (i < a.n) {
    const uint64_t dr = ((uint64_t)a.ids[i] << a.comp_code_bits) + a.comp;
    const uint64_t ind = a.rev[dr & 4095u];
    const uint64_t tuple = ((dr >> a.pf_bits) << a.inner_bits) + ind;
    const uint64_t hom = ((1ull << a.hob) - 1ull) << a.inner_bits;
    uint64_t uni = (tuple & (hom << a.hob)) + ((tuple & hom) >> a.inner_bits) + ((tuple & ((1ull << a.inner_bits) - 1ull)) << a.hob);
    uint8_t *line = lines + threadIdx.x * W;
    for (uint32_t j = 0; j < a.TL; j++) {
      const uint32_t c = (uint32_t)uni & 3u;
      line[a.TL - 1u - j] = (uint8_t)(c == 0u ? 'A' : c == 1u ? 'C' : c == 2u ? 'G' : 'T'); /* Mapbase, global_basic.c:70 */
      uni >>= 2;
    }
    line[a.TL] = (uint8_t)'\n';
  }
  __syncthreads();
  const uint32_t nvec = MK_BR_REV_IDS * W / 16u; /* 16 * W */
  uint4 *dst = out + (uint64_t)blockIdx.x * nvec;
  for (uint32_t v = threadIdx.x; v < nvec; v += MK_BR_REV_IDS) dst[v] = lines4[v];
}

} /* namespace */

struct mk_byread {
  int device = 0, num_cu = 256;
  hipStream_t stream = nullptr;
  bool begun = false, finished = false, have_rev = false;
  mk_params P;
  mk_keyparams kp;
  uint32_t ncarry = 0;
  int32_t *d_shuf = nullptr;
  uint64_t shuf_cap = 0;
  uint32_t *d_accept_bits = nullptr;
  uint64_t bits_cap = 0;
  uint32_t *d_rev = nullptr;
  uint8_t *d_text = nullptr, *d_stream = nullptr;
  mk_fa_sum *d_sum = nullptr;
  uint32_t *d_chunk = nullptr, *d_ids = nullptr, *d_rec = nullptr;
  unsigned long long *d_idx = nullptr;
  uint64_t idx_cap = 0;
  mk_br_state *d_st = nullptr, *h_st = nullptr;
  uint32_t *h_ids = nullptr;
  unsigned long long *h_idx = nullptr;
  uint64_t h_idx_cap = 0;
  /* what the last push left for mk_byread_take */
  uint64_t n_ids[MK_BR_MAXC] = {0}, start[MK_BR_MAXC + 1] = {0}, n_index = 0, nrec = 0;
  /* the file so far */
  uint64_t before[MK_BR_MAXC] = {0}, records = 0, text_bytes = 0;
  /* reverse */
  uint32_t *d_rids = nullptr;
  uint4 *d_rtext = nullptr;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  double emit_ms = 0.0, reverse_ms = 0.0;
  char err[256] = {0};
};

static thread_local char mk_byread_create_err[256];

static int mk_br_fail(mk_byread *b, int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b ? b->err : mk_byread_create_err, 256, fmt, ap);
  va_end(ap);
  return code;
}

#define MK_BR_HIP(b, call)                                                                          \
  do {                                                                                              \
    hipError_t _r = (call);                                                                         \
    if (_r != hipSuccess) return mk_br_fail(b, MK_ERR_HIP, "%s: %s", #call, hipGetErrorString(_r)); \
  } while (0)

template <class T>
static int mk_br_grow(mk_byread *b, T **p, uint64_t *cap, uint64_t need) {
  if (need == 0) need = 1;
  if (need <= *cap && *p) return MK_OK;
  (void)hipFree(*p);
  *p = nullptr; *cap = 0;
  const uint64_t c = need + need / 8 + 256;
  MK_BR_HIP(b, mk_dev_alloc(p, c * sizeof(T)));
  *cap = c;
  return MK_OK;
}

extern "C" int mk_byread_create(int device, mk_byread **out) {
  if (!out) return MK_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return mk_br_fail(nullptr, MK_ERR_NO_DEVICE, "no HIP device: mk_byread has no CPU path");
  if (device < 0 || device >= ndev) return mk_br_fail(nullptr, MK_ERR_NO_DEVICE, "device %d out of range (0..%d)", device, ndev - 1);
  mk_byread *b = new (std::nothrow) mk_byread();
  if (!b) return MK_ERR_NOMEM;
  b->device = device;
  hipDeviceProp_t prop;
  if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) {
    delete b;
    return mk_br_fail(nullptr, MK_ERR_NO_DEVICE, "hipSetDevice(%d) failed", device);
  }
  b->num_cu = prop.multiProcessorCount;
  const size_t CH = MK_BYREAD_MAX_PUSH, nchunks = CH / MK_BR_CHUNK, nseg = CH / MK_FA_SEG;
  hipError_t r = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
  /* the text and the stream end in slack: the staging loads of a segment / chunk run up to 1 KiB + 32 bytes past the data */
  if (r == hipSuccess) r = mk_dev_alloc(&b->d_text, CH + 2048);
  if (r == hipSuccess) r = mk_dev_alloc(&b->d_stream, CH + 2048 + 64);
  if (r == hipSuccess) r = mk_dev_alloc(&b->d_sum, nseg * sizeof(mk_fa_sum));
  if (r == hipSuccess) r = mk_dev_alloc(&b->d_chunk, (size_t)MK_BR_ROWS * nchunks * sizeof(uint32_t));
  if (r == hipSuccess) r = mk_dev_alloc(&b->d_ids, CH * sizeof(uint32_t));
  if (r == hipSuccess) r = mk_dev_alloc(&b->d_rec, CH * sizeof(uint32_t));
  if (r == hipSuccess) r = mk_dev_alloc(&b->d_st, sizeof(mk_br_state));
  if (r == hipSuccess) r = mk_dev_alloc(&b->d_rev, 4096 * sizeof(uint32_t));
  if (r == hipSuccess) r = mk_pin_alloc(&b->h_st, sizeof(mk_br_state), hipHostMallocDefault);
  if (r == hipSuccess) r = mk_pin_alloc(&b->h_ids, CH * sizeof(uint32_t), hipHostMallocDefault);
  for (int i = 0; i < 6 && r == hipSuccess; i++) r = hipEventCreate(&b->ev[i]);
  if (r != hipSuccess) {
    mk_br_fail(nullptr, MK_ERR_NOMEM, "byread allocation: %s", hipGetErrorString(r));
    mk_byread_destroy(b);
    return MK_ERR_NOMEM;
  }
  *out = b;
  return MK_OK;
}

extern "C" int mk_byread_destroy(mk_byread *b) {
  if (!b) return MK_OK;
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  void *dev[] = {b->d_shuf, b->d_accept_bits, b->d_rev, b->d_text, b->d_stream, b->d_sum, b->d_chunk, b->d_ids, b->d_rec, b->d_idx,
                 b->d_st, b->d_rids, b->d_rtext};
  for (void *p : dev) (void)hipFree(p);
  void *pin[] = {b->h_st, b->h_ids, b->h_idx};
  for (void *p : pin) if (p) (void)hipHostFree(p);
  for (hipEvent_t e : b->ev) if (e) (void)hipEventDestroy(e);
  if (b->stream) (void)hipStreamDestroy(b->stream);
  delete b;
  return MK_OK;
}

extern "C" const char *mk_byread_last_error(const mk_byread *b) { return b ? b->err : mk_byread_create_err; }

/* seq2co_global_var_initial() (iseq2comem.c:54-86) for the walk; the inverse table of command_reverse.c:150-160 for mk_reverse_ids */
extern "C" int mk_byread_begin(mk_byread *b, const mk_params *p) {
  if (!b || !p || !p->shuf_table) return MK_ERR_ARG;
  if (p->component_num < 1 || p->component_num > (int32_t)MK_BR_MAXC) return mk_br_fail(b, MK_ERR_ARG, "%d components (at most 16)", p->component_num);
  if (p->TL < 2 || p->TL > 32 || p->shuf_len != (1ull << (4 * p->subk))) return mk_br_fail(b, MK_ERR_ARG, "parameters not from mk_params_init");
  MK_BR_HIP(b, hipSetDevice(b->device));
  b->P = *p;
  mk_keyparams &kp = b->kp;
  kp.tupmask = p->tupmask; kp.domask = p->domask; kp.undomask = p->undomask;
  kp.lowmask = (1ull << (2 * p->half_outctx_len)) - 1ull;
  kp.TL = (uint32_t)p->TL; kp.crvsaddmove = (uint32_t)p->crvsaddmove;
  kp.out2 = 2u * (uint32_t)p->half_outctx_len;
  kp.key_lshift = 2u * (uint32_t)p->TL - 4u * (uint32_t)p->half_outctx_len;
  kp.dr4 = 4u * (uint32_t)p->drlevel;
  kp.dim_start = p->dim_start; kp.dim_end = p->dim_end;
  kp.S = p->hashsize;
  b->ncarry = kp.TL - 1u;
  const uint64_t L = p->shuf_len, words = (L + 31u) / 32u;
  int rc;
  if ((rc = mk_br_grow(b, &b->d_shuf, &b->shuf_cap, L)) || (rc = mk_br_grow(b, &b->d_accept_bits, &b->bits_cap, words))) return rc;
  MK_BR_HIP(b, hipMemcpyAsync(b->d_shuf, p->shuf_table, L * sizeof(int32_t), hipMemcpyHostToDevice, b->stream));
  unsigned blocks = (unsigned)((words + 255u) / 256u);
  if (blocks > (unsigned)b->num_cu * 8u) blocks = (unsigned)b->num_cu * 8u;
  hipLaunchKernelGGL(mk_br_accept_kernel, dim3(blocks ? blocks : 1u), dim3(256), 0, b->stream, (const int32_t *)b->d_shuf, L, p->dim_start, p->dim_end,
                     b->d_accept_bits);
  hipLaunchKernelGGL(mk_br_reset_kernel, dim3(1), dim3(64), 0, b->stream, b->d_stream, b->d_st, b->ncarry);
  MK_BR_HIP(b, hipGetLastError());
  /* rev_shuf_arr: the reference wants exactly 4096 entries below 4096 (command_reverse.c:154-160) */
  static thread_local uint32_t rev[4096];
  uint64_t count = 0;
  for (uint64_t i = 0; i < L; i++) {
    const int32_t v = p->shuf_table[i];
    if (v >= 0 && v < 4096) { rev[v] = (uint32_t)i; count++; }
  }
  b->have_rev = count == 4096;
  if (b->have_rev) MK_BR_HIP(b, hipMemcpyAsync(b->d_rev, rev, sizeof rev, hipMemcpyHostToDevice, b->stream));
  MK_BR_HIP(b, hipStreamSynchronize(b->stream));
  for (uint32_t c = 0; c < MK_BR_MAXC; c++) { b->before[c] = 0; b->n_ids[c] = 0; b->start[c] = 0; }
  b->start[MK_BR_MAXC] = 0;
  b->records = 0; b->text_bytes = 0; b->n_index = 0; b->nrec = 0;
  b->emit_ms = 0.0; b->reverse_ms = 0.0;
  b->begun = true; b->finished = false;
  return MK_OK;
}

/* the byte loop of reads2mco(), iseq2comem.c:127-200, over the next n bytes of the file */
extern "C" int mk_byread_push_text(mk_byread *b, const void *text, uint64_t n, int final) {
  if (!b || (n && !text)) return MK_ERR_ARG;
  if (!b->begun || b->finished) return mk_br_fail(b, MK_ERR_STATE, "mk_byread_push_text outside begin .. final push");
  if (n > MK_BYREAD_MAX_PUSH) return mk_br_fail(b, MK_ERR_ARG, "%llu bytes in one push (at most %u)", (unsigned long long)n, (unsigned)MK_BYREAD_MAX_PUSH);
  MK_BR_HIP(b, hipSetDevice(b->device));
  const uint32_t C = (uint32_t)b->P.component_num;
  uint64_t g = 0; /* '>' bytes of this push */
  for (uint32_t c = 0; c < MK_BR_MAXC; c++) b->n_ids[c] = 0;
  for (uint32_t c = 0; c <= MK_BR_MAXC; c++) b->start[c] = 0;
  mk_br_args a;
  a.stream = b->d_stream; a.st = b->d_st; a.kp = b->kp; a.accept_bits = b->d_accept_bits; a.shuf = b->d_shuf;
  a.comp_num = C; a.comp_code_bits = (uint32_t)b->P.comp_code_bits;
  a.nchunks = (uint32_t)((n + MK_BR_CHUNK - 1u) / MK_BR_CHUNK);
  if (n) {
    const uint64_t nseg = (n + MK_FA_SEG - 1u) / MK_FA_SEG;
    const unsigned fa_blocks = (unsigned)((nseg + MK_FA_WAVES - 1u) / MK_FA_WAVES), br_blocks = (a.nchunks + MK_BR_WAVES - 1u) / MK_BR_WAVES;
    MK_BR_HIP(b, hipMemcpyAsync(b->d_text, text, n, hipMemcpyHostToDevice, b->stream));
    MK_BR_HIP(b, hipEventRecord(b->ev[0], b->stream));
    hipLaunchKernelGGL(mk_fa_summary_kernel, dim3(fa_blocks), dim3(64 * MK_FA_WAVES), 0, b->stream, (const uint8_t *)b->d_text, n, b->d_sum);
    hipLaunchKernelGGL(mk_br_fa_scan_kernel, dim3(1), dim3(1024), 0, b->stream, b->d_sum, nseg, b->d_st);
    hipLaunchKernelGGL(mk_fa_emit_kernel, dim3(fa_blocks), dim3(64 * MK_FA_WAVES), 0, b->stream, (const uint8_t *)b->d_text, n, (const mk_fa_sum *)b->d_sum,
                       b->d_stream, (unsigned long long)b->ncarry);
    hipLaunchKernelGGL(mk_br_count_kernel, dim3(br_blocks), dim3(64 * MK_BR_WAVES), 0, b->stream, a, b->d_chunk);
    hipLaunchKernelGGL(mk_br_scan_kernel, dim3(C + 1u), dim3(1024), 0, b->stream, b->d_chunk, a.nchunks, C, b->d_st);
    MK_BR_HIP(b, hipGetLastError());
    MK_BR_HIP(b, hipEventRecord(b->ev[1], b->stream));
  }
  /* the totals decide the sizes of everything behind them: 160 bytes come to the host once per push */
  MK_BR_HIP(b, hipMemcpyAsync(b->h_st, b->d_st, sizeof(mk_br_state), hipMemcpyDeviceToHost, b->stream));
  MK_BR_HIP(b, hipStreamSynchronize(b->stream));
  uint64_t total = 0;
  if (n) {
    for (uint32_t c = 0; c < C; c++) { b->n_ids[c] = b->h_st->totals[c]; b->start[c] = total; total += b->n_ids[c]; }
    for (uint32_t c = C; c <= MK_BR_MAXC; c++) b->start[c] = total;
    g = b->h_st->totals[MK_BR_MAXC];
  }
  if (final && b->h_st->in_header)
    return mk_br_fail(b, MK_ERR_FORMAT, "the text ends inside a '>' line (the reference gives up there, iseq2comem.c:161-170)");
  const uint64_t nrec = g + 1u; /* records this push touches: the open one and one per '>' */
  int rc;
  {
    const uint64_t need = (uint64_t)C * nrec;
    if (need > b->h_idx_cap || !b->h_idx) {
      if (b->h_idx) (void)hipHostFree(b->h_idx);
      b->h_idx = nullptr; b->h_idx_cap = 0;
      const uint64_t c = need + need / 8 + 256;
      MK_BR_HIP(b, mk_pin_alloc(&b->h_idx, c * sizeof(unsigned long long), hipHostMallocDefault));
      b->h_idx_cap = c;
    }
    if ((rc = mk_br_grow(b, &b->d_idx, &b->idx_cap, need))) return rc;
  }
  if (n) {
    const unsigned br_blocks = (a.nchunks + MK_BR_WAVES - 1u) / MK_BR_WAVES;
    mk_br_index_args x;
    for (uint32_t c = 0; c < MK_BR_MAXC; c++) { x.before[c] = b->before[c]; x.start[c] = (uint32_t)b->start[c]; }
    x.start[MK_BR_MAXC] = (uint32_t)b->start[MK_BR_MAXC];
    uint64_t ib = ((uint64_t)C * nrec + 255u) / 256u;
    if (ib > (uint64_t)b->num_cu * 8u) ib = (uint64_t)b->num_cu * 8u;
    MK_BR_HIP(b, hipEventRecord(b->ev[2], b->stream));
    hipLaunchKernelGGL(mk_br_write_kernel, dim3(br_blocks), dim3(64 * MK_BR_WAVES), 0, b->stream, a, (const uint32_t *)b->d_chunk, b->d_ids, b->d_rec);
    hipLaunchKernelGGL(mk_br_index_kernel, dim3((unsigned)ib), dim3(256), 0, b->stream, x, (const uint32_t *)b->d_rec, C, nrec, b->d_idx);
    hipLaunchKernelGGL(mk_br_carry_kernel, dim3(1), dim3(64), 0, b->stream, b->d_stream, (const mk_br_state *)b->d_st, b->ncarry);
    MK_BR_HIP(b, hipGetLastError());
    MK_BR_HIP(b, hipEventRecord(b->ev[3], b->stream));
    if (total) MK_BR_HIP(b, hipMemcpyAsync(b->h_ids, b->d_ids, total * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
    MK_BR_HIP(b, hipMemcpyAsync(b->h_idx, b->d_idx, (uint64_t)C * nrec * sizeof(unsigned long long), hipMemcpyDeviceToHost, b->stream));
    MK_BR_HIP(b, hipStreamSynchronize(b->stream));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, b->ev[0], b->ev[1]) == hipSuccess) b->emit_ms += ms;
    if (hipEventElapsedTime(&ms, b->ev[2], b->ev[3]) == hipSuccess) b->emit_ms += ms;
  } else {
    for (uint32_t c = 0; c < C; c++) b->h_idx[c] = b->before[c]; /* nrec == 1: the open record, nothing added */
  }
  for (uint32_t c = 0; c < C; c++) b->before[c] += b->n_ids[c];
  b->nrec = nrec;
  b->n_index = final ? nrec : g; /* a record is complete when the next '>' has been seen, the last one at the end of the file */
  b->records += g;
  b->text_bytes += n;
  if (final) b->finished = true;
  return MK_OK;
}

/* fwrite(&newid, ..) to outf[c] (iseq2comem.c:197-198) and the cumulative loop (:202-207), for what the last push added */
extern "C" int mk_byread_take(mk_byread *b, uint32_t component, const uint32_t **ids, uint64_t *n_ids, const uint64_t **index, uint64_t *n_index) {
  if (!b || !ids || !n_ids || !index || !n_index) return MK_ERR_ARG;
  if (!b->begun) return mk_br_fail(b, MK_ERR_STATE, "mk_byread_take before mk_byread_begin");
  if (component >= (uint32_t)b->P.component_num) return mk_br_fail(b, MK_ERR_ARG, "component %u of %d", component, b->P.component_num);
  *ids = b->h_ids + b->start[component];
  *n_ids = b->n_ids[component];
  *index = (const uint64_t *)(b->h_idx + (uint64_t)component * b->nrec);
  *n_index = b->n_index;
  return MK_OK;
}

extern "C" int mk_byread_finish(mk_byread *b, uint64_t *records, uint64_t *total_ids, double *kernel_ms) {
  if (!b) return MK_ERR_ARG;
  if (!b->begun || !b->finished) return mk_br_fail(b, MK_ERR_STATE, "mk_byread_finish before the final push");
  if (records) *records = b->records;
  if (total_ids) {
    uint64_t t = 0;
    for (int c = 0; c < b->P.component_num; c++) t += b->before[c];
    *total_ids = t;
  }
  if (kernel_ms) *kernel_ms = b->emit_ms;
  b->begun = false;
  for (uint32_t c = 0; c < MK_BR_MAXC; c++) b->n_ids[c] = 0;
  b->n_index = 0;
  return MK_OK;
}

/* core_reverse2unituple() + the kstring loop + fprintf, command_reverse.c:214-219 / :342-348 */
extern "C" int mk_reverse_ids(mk_byread *b, const uint32_t *ids, uint64_t n, uint32_t component, char *out_text) {
  if (!b || (n && (!ids || !out_text))) return MK_ERR_ARG;
  if (!b->P.shuf_table) return mk_br_fail(b, MK_ERR_STATE, "mk_reverse_ids before mk_byread_begin");
  if (!b->have_rev) return mk_br_fail(b, MK_ERR_FORMAT, "the .shuf table does not have 4096 entries below 4096 (command_reverse.c:160)");
  if (component >= (uint32_t)b->P.component_num) return mk_br_fail(b, MK_ERR_ARG, "component %u of %d", component, b->P.component_num);
  MK_BR_HIP(b, hipSetDevice(b->device));
  if (!b->d_rids) MK_BR_HIP(b, mk_dev_alloc(&b->d_rids, (size_t)MK_BR_REV_BATCH * sizeof(uint32_t)));
  if (!b->d_rtext) MK_BR_HIP(b, mk_dev_alloc(&b->d_rtext, (size_t)MK_BR_REV_BATCH * 33u)); /* whole workgroups of 256 lines */
  mk_br_rev_args a;
  a.ids = b->d_rids; a.rev = b->d_rev; a.comp = component;
  a.comp_code_bits = (uint32_t)b->P.comp_code_bits;
  a.pf_bits = 4u * (uint32_t)(b->P.subk - b->P.drlevel);
  a.inner_bits = 4u * (uint32_t)b->P.subk;
  a.hob = 2u * (uint32_t)(b->P.k - b->P.subk);
  a.TL = (uint32_t)b->P.TL;
  const uint64_t W = a.TL + 1u;
  for (uint64_t done = 0; done < n; done += MK_BR_REV_BATCH) {
    const uint64_t m = n - done < MK_BR_REV_BATCH ? n - done : MK_BR_REV_BATCH;
    a.n = m;
    MK_BR_HIP(b, hipMemcpyAsync(b->d_rids, ids + done, m * sizeof(uint32_t), hipMemcpyHostToDevice, b->stream));
    MK_BR_HIP(b, hipEventRecord(b->ev[4], b->stream));
    hipLaunchKernelGGL(mk_br_reverse_kernel, dim3((unsigned)((m + MK_BR_REV_IDS - 1u) / MK_BR_REV_IDS)), dim3(MK_BR_REV_IDS), 0, b->stream, a, b->d_rtext);
    MK_BR_HIP(b, hipGetLastError());
    MK_BR_HIP(b, hipEventRecord(b->ev[5], b->stream));
    MK_BR_HIP(b, hipMemcpyAsync(out_text + done * W, b->d_rtext, m * W, hipMemcpyDeviceToHost, b->stream));
    MK_BR_HIP(b, hipStreamSynchronize(b->stream));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, b->ev[4], b->ev[5]) == hipSuccess) b->reverse_ms += ms;
  }
  return MK_OK;
}

extern "C" int mk_byread_last_kernel_ms(mk_byread *b, double *emit_ms, double *reverse_ms) {
  if (!b) return MK_ERR_ARG;
  if (emit_ms) *emit_ms = b->emit_ms;
  if (reverse_ms) *reverse_ms = b->reverse_ms;
  return MK_OK;
}
