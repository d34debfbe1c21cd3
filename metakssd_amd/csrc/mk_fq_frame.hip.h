/*
 * mk_fq_frame.hip.h -- FASTQ framing of text already in HBM (gfx950, wave64): the kernels, their launches, and mk_fq_framer, the host
 * side every caller runs (BGZF route, gunzip route, test entries).  No deflate here; mk_inflate.hip includes it behind mk_lds_fence(), mk_grow().
 *   mk_fq_count_kernel   newlines per 4 KiB tile of the text and the last one's place
 *   mk_fq_scan_kernel    one workgroup: exclusive prefix over the tiles (= the line number at every tile's start), the number of
 *                        complete records, the first member with a bad status
 *   mk_fq_reduce_kernel  a wave per tile, a lane per 64 bytes: every newline's line number and the newline in front of it (from the
 *                        lanes' bit masks; from the text in front of the tile only for the tile's first) -> the longest line, the
 *                        longest sequence line of a complete record, the end of the last complete record
 *   mk_fq_rows_kernel    the same walk; the sequence lines found are copied by the whole wave, four bytes a lane, zero-padded
 *   mk_fq_carry_kernel   what lies behind the last complete record moves in front of the next chunk's text (launched by the callers:
 *                        where it goes is theirs to say)
 * The framing rule is mk_fastq_frame_range's (host/mk_frontend.c) and depends on line numbers only: record r is lines 4r..4r+3, it
 * gives a row iff its fourth line has at least one byte, the row is line 4r+1 with its '\n'.  (One difference, outside the contract
 * either way: a line of 4095+ characters is refused wherever it stands, also in a last record that lacks lines.)
 *   mk_fq_reduce_q_kernel / mk_fq_rows_q_kernel / mk_fq_first_q_kernel
 *                        the same for fastq2co's reader (dist without -A: -n, -Q), whose rule is mk_fastq_frame_q_range's: record r
 *                        gives a row iff all four of its lines end in '\n', the row is line 4r+1 with the bases whose byte of line
 *                        4r+3 is below -Q written as 'N'.  The reduce walk also leaves where every record's quality line starts and
 *                        how long it is (8 bytes a record); the rows kernel masks while it copies.  The first record of a file that
 *                        holds no complete one is walked all the same (iseq2comem.c:343-349): one wave does that serially.  No
 *                        windows: a line of 4095+ characters is refused, the caller takes the host framer for such a file.
 * Bound of each kernel: DESIGN.md 4.10, 4.12.
 */
#pragma once

#define MK_FQ_TILE 4096u       /* text bytes per wave */
#define MK_FQ_WAVES 4u
#define MK_FQ_CARRY 16384u     /* room in front of a chunk's text: four lines of at most 4095 bytes (more means a line that long) */
#define MK_FQ_LINE_MAX 4096u   /* MK_FQ_LEN: a line of this many bytes with its '\n' is refused (mk_frontend.c) */

namespace {

struct mk_fq_res {
  uint32_t nl, nrec, consumed, maxline, maxseq; /* text coordinates */
  uint32_t bad_block, bad_status;               /* first member with a status != 0 (0xffffffff: none) */
  uint32_t pad;
};

/* ---- FASTQ framing of text in HBM ---------------------------------------------------------------------------------------------
 * `buf` is a 16-byte aligned buffer, the text is buf[t0, e1); tiles and positions are in buffer coordinates, the buffer is
 * allocated up to the end of the last tile (what lies outside [t0, e1) is loaded and masked, never used). */
__device__ __forceinline__ uint32_t mk_nl4(uint32_t w) { /* bit k: byte k of w is '\n' */
  const uint32_t x = w ^ 0x0a0a0a0au;
  const uint32_t t = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
  return ((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u);
}
__device__ __forceinline__ uint64_t mk_fq_mask(const uint8_t *buf, uint32_t b, uint32_t t0, uint32_t e1) {
  if (b >= e1 || b + 64u <= t0) return 0ull;
  uint64_t m = 0;
  const uint4 *p = (const uint4 *)(buf + b);
  for (uint32_t q = 0; q < 4u; q++) {
    const uint4 v = p[q];
    const uint64_t n16 = (uint64_t)(mk_nl4(v.x) | mk_nl4(v.y) << 4 | mk_nl4(v.z) << 8 | mk_nl4(v.w) << 12);
    m |= n16 << (16u * q);
  }
  if (t0 > b) m &= ~0ull << (t0 - b);
  if (e1 - b < 64u) m &= (1ull << (e1 - b)) - 1ull;
  return m;
}
__device__ __forceinline__ uint32_t mk_wave_sum(uint32_t v) {
  for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
  return v;
}
__device__ __forceinline__ uint32_t mk_wave_max(uint32_t v) {
  for (int o = 32; o; o >>= 1) { const uint32_t u = (uint32_t)__shfl_xor((int)v, o); v = u > v ? u : v; }
  return v;
}

__device__ __forceinline__ uint32_t mk_fq_stride_dev(uint32_t need) { return MK_ROW_PITCH(need); }

__global__ void __launch_bounds__(64 * MK_FQ_WAVES) mk_fq_count_kernel(const uint8_t *buf, uint32_t t0, uint32_t e1, uint32_t ntiles,
                                                                       uint32_t *tile_cnt, uint32_t *tile_last) {
  const uint32_t lane = threadIdx.x & 63u, tile = blockIdx.x * MK_FQ_WAVES + (threadIdx.x >> 6);
  if (tile >= ntiles) return;
  const uint32_t b = tile * MK_FQ_TILE + 64u * lane;
  const uint64_t m = mk_fq_mask(buf, b, t0, e1);
  const uint32_t c = mk_wave_sum((uint32_t)__popcll(m));
  const uint32_t last = mk_wave_max(m ? b + (63u - (uint32_t)__clzll(m)) + 1u : 0u); /* position + 1; 0: none */
  if (lane == 0u) { tile_cnt[tile] = c; tile_last[tile] = last; }
}

/* one workgroup of 1024 threads: tile_cnt becomes its exclusive prefix; the totals of the chunk */
__global__ void __launch_bounds__(1024) mk_fq_scan_kernel(uint32_t *tile_cnt, const uint32_t *tile_last, uint32_t ntiles, uint32_t t0, uint32_t e1,
                                                          int final, const uint32_t *status, uint32_t nblocks, mk_fq_res *res) {
  __shared__ uint32_t sums[1024];
  __shared__ uint32_t s_last, s_bad;
  const uint32_t t = threadIdx.x;
  if (t == 0u) { s_last = 0u; s_bad = 0xffffffffu; }
  __syncthreads();
  const uint32_t per = (ntiles + 1023u) / 1024u;
  const uint32_t lo = t * per < ntiles ? t * per : ntiles, hi = lo + per < ntiles ? lo + per : ntiles;
  uint32_t s = 0, lastp = 0;
  for (uint32_t i = lo; i < hi; i++) { s += tile_cnt[i]; const uint32_t l = tile_last[i]; lastp = l > lastp ? l : lastp; }
  sums[t] = s;
  if (lastp) atomicMax(&s_last, lastp);
  for (uint32_t i = t; i < nblocks; i += 1024u) if (status[i]) atomicMin(&s_bad, i);
  __syncthreads();
  for (uint32_t d = 1; d < 1024u; d <<= 1) { /* inclusive scan */
    const uint32_t v = t >= d ? sums[t - d] : 0u;
    __syncthreads();
    sums[t] += v;
    __syncthreads();
  }
  uint32_t run = sums[t] - s;
  for (uint32_t i = lo; i < hi; i++) { const uint32_t c = tile_cnt[i]; tile_cnt[i] = run; run += c; }
  if (t == 0u) {
    const uint32_t n = e1 - t0, nl = sums[1023];
    const uint32_t partial = s_last ? e1 - s_last : n; /* bytes behind the last newline */
    const uint32_t lines = nl + (uint32_t)(final && partial > 0u);
    mk_fq_res r;
    r.nl = nl;
    r.nrec = (final ? lines : nl) / 4u;
    r.consumed = final ? n : 0u; /* (not final: the reduce kernel's thread that meets newline 4 * nrec - 1 says) */
    r.maxline = final ? partial : 0u;
    r.maxseq = 0u;
    r.bad_block = s_bad;
    r.bad_status = s_bad != 0xffffffffu ? status[s_bad] : 0u;
    r.pad = 0u;
    *res = r;
  }
}

/* f(j, q, p) for every newline of the wave's tile, in the lane that holds it: p its position, j its number in the text (it ends
 * line j), q the position of the newline in front of it (t0 - 1 for j == 0).  A line of more than MK_FQ_LINE_MAX bytes may be
 * reported shorter, but never below MK_FQ_LINE_MAX + 1. */
template <class F>
__device__ __forceinline__ void mk_fq_walk(const uint8_t *buf, uint32_t t0, uint32_t e1, uint32_t tile, uint32_t base, uint32_t lane, F f) {
  const uint32_t b = tile * MK_FQ_TILE + 64u * lane;
  uint64_t m = mk_fq_mask(buf, b, t0, e1);
  const uint64_t have = __ballot(m != 0ull);
  const uint32_t pc = (uint32_t)__popcll(m);
  uint32_t ex = pc;
  for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)ex, o); if ((int)lane >= o) ex += u; }
  ex -= pc;
  const uint64_t before = have & ((1ull << lane) - 1ull);
  const int src = before ? 63 - __clzll(before) : 0;
  const uint32_t mlo = (uint32_t)__shfl((int)(uint32_t)m, src), mhi = (uint32_t)__shfl((int)(uint32_t)(m >> 32), src);
  if (!m) return;
  uint32_t j = base + ex;
  int32_t q;
  if (before) q = (int32_t)(tile * MK_FQ_TILE + 64u * (uint32_t)src + (63u - (uint32_t)__clzll((uint64_t)mhi << 32 | mlo)));
  else if (j == 0u) q = (int32_t)t0 - 1;
  else { /* the tile's first newline: its predecessor lies in front of the tile, at most a line away */
    const int32_t s = (int32_t)(tile * MK_FQ_TILE) - 1;
    int32_t lim = s - (int32_t)MK_FQ_LINE_MAX;
    if (lim < (int32_t)t0) lim = (int32_t)t0;
    q = s;
    while (q >= lim && buf[q] != (uint8_t)'\n') q--;
  }
  while (m) {
    const uint32_t p = b + (uint32_t)__builtin_ctzll(m);
    f(j, q, p);
    q = (int32_t)p;
    j++;
    m &= m - 1ull;
  }
}

__global__ void __launch_bounds__(64 * MK_FQ_WAVES) mk_fq_reduce_kernel(const uint8_t *buf, uint32_t t0, uint32_t e1, uint32_t ntiles,
                                                                        const uint32_t *tile_base, int final, mk_fq_res *res) {
  const uint32_t lane = threadIdx.x & 63u, tile = blockIdx.x * MK_FQ_WAVES + (threadIdx.x >> 6);
  if (tile >= ntiles) return;
  const uint32_t nrec = res->nrec;
  uint32_t maxline = 0, maxseq = 0;
  mk_fq_walk(buf, t0, e1, tile, tile_base[tile], lane, [&](uint32_t j, int32_t q, uint32_t p) {
    const uint32_t len = (uint32_t)((int32_t)p - q);
    maxline = len > maxline ? len : maxline;
    if ((j & 3u) == 1u && (j >> 2) < nrec) maxseq = len > maxseq ? len : maxseq;
    if (!final && nrec && j == 4u * nrec - 1u) res->consumed = p + 1u - t0;
  });
  maxline = mk_wave_max(maxline);
  maxseq = mk_wave_max(maxseq);
  if (lane == 0u) {
    if (maxline) atomicMax(&res->maxline, maxline);
    if (maxseq) atomicMax(&res->maxseq, maxseq);
  }
}

/* rows [r0, r1) of the chunk: row r is line 4r + 1 with its '\n', zero-padded to `stride` */
__global__ void __launch_bounds__(64 * MK_FQ_WAVES) mk_fq_rows_kernel(const uint8_t *buf, uint32_t t0, uint32_t e1, uint32_t ntiles,
                                                                      const uint32_t *tile_base, uint32_t r0, uint32_t r1, uint32_t stride,
                                                                      uint8_t *rows) {
  __shared__ uint32_t ev_start[MK_FQ_WAVES][MK_FQ_TILE / 4], ev_len[MK_FQ_WAVES][MK_FQ_TILE / 4], ev_row[MK_FQ_WAVES][MK_FQ_TILE / 4];
  __shared__ uint32_t ev_n[MK_FQ_WAVES];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, tile = blockIdx.x * MK_FQ_WAVES + wave;
  if (tile >= ntiles) return;
  if (lane == 0u) ev_n[wave] = 0u;
  mk_lds_fence();
  /* sequence lines end at least four bytes apart: a tile holds at most MK_FQ_TILE / 4 of them */
  mk_fq_walk(buf, t0, e1, tile, tile_base[tile], lane, [&](uint32_t j, int32_t q, uint32_t p) {
    const uint32_t r = j >> 2;
    if ((j & 3u) != 1u || r < r0 || r >= r1) return;
    const uint32_t at = atomicAdd(&ev_n[wave], 1u);
    ev_start[wave][at] = (uint32_t)(q + 1);
    ev_len[wave][at] = (uint32_t)((int32_t)p - q);
    ev_row[wave][at] = r - r0;
  });
  mk_lds_fence();
  const uint32_t n = ev_n[wave];
  for (uint32_t e = 0; e < n; e++) {
    const uint32_t start = ev_start[wave][e], row = ev_row[wave][e];
    uint32_t len = ev_len[wave][e];
    if (len > stride) len = stride; /* (cannot happen: the stride comes from the longest of these lines) */
    uint32_t *dst = (uint32_t *)(rows + (uint64_t)row * stride);
    for (uint32_t o = 4u * lane; o < stride; o += 256u) {
      uint32_t w = 0;
      for (uint32_t k = 0; k < 4u; k++) if (o + k < len) w |= (uint32_t)buf[start + o + k] << (8u * k);
      dst[o >> 2] = w;
    }
  }
}

/* ---- the same for fastq2co's reader (mk_fastq_frame_q_range, one row a record) -------------------------------------------------
 * The scan kernel is launched with final == 0, so res->nrec = newlines / 4: only a record whose four lines are all terminated is a
 * row, final call or not.  This walk adds what the rows kernel needs: qinfo[2r] = where record r's quality line starts (behind
 * newline 4r + 2), qinfo[2r + 1] = its length with its '\n' (newline 4r + 3 minus the one in front of it), for r < nrec; both
 * newlines exist for such a record, so both words are written, and start + length <= e1.  final: what lies behind the last newline
 * is a line too (the longest-line test sees it).  Stores: res, and qinfo below 2 * min(nrec, qcap). */
__global__ void __launch_bounds__(64 * MK_FQ_WAVES) mk_fq_reduce_q_kernel(const uint8_t *buf, uint32_t t0, uint32_t e1, uint32_t ntiles,
                                                                          const uint32_t *tile_base, int final, mk_fq_res *res,
                                                                          uint32_t *qinfo, uint32_t qcap) {
  const uint32_t lane = threadIdx.x & 63u, tile = blockIdx.x * MK_FQ_WAVES + (threadIdx.x >> 6);
  if (tile >= ntiles) return;
  const uint32_t nl = res->nl;
  uint32_t nrec = res->nrec;
  if (nrec > qcap) nrec = qcap; /* (cannot happen: qcap >= text / 4 >= newlines / 4) */
  uint32_t maxline = 0, maxseq = 0;
  mk_fq_walk(buf, t0, e1, tile, tile_base[tile], lane, [&](uint32_t j, int32_t q, uint32_t p) {
    const uint32_t len = (uint32_t)((int32_t)p - q), r = j >> 2, w = j & 3u;
    maxline = len > maxline ? len : maxline;
    if (final && j + 1u == nl) { const uint32_t tail = e1 - (p + 1u); maxline = tail > maxline ? tail : maxline; }
    if (r >= nrec) return;
    if (w == 1u) maxseq = len > maxseq ? len : maxseq;
    else if (w == 2u) qinfo[2u * r] = p + 1u;
    else if (w == 3u) {
      qinfo[2u * r + 1u] = len;
      if (r + 1u == nrec) res->consumed = p + 1u - t0;
    }
  });
  maxline = mk_wave_max(maxline);
  maxseq = mk_wave_max(maxseq);
  if (lane == 0u) {
    if (maxline) atomicMax(&res->maxline, maxline);
    if (maxseq) atomicMax(&res->maxseq, maxseq);
  }
}

/* base i of a row: the sequence byte, or 'N' when its quality byte (signed, 0 behind the quality line's end) is below qmin */
__device__ __forceinline__ uint32_t mk_fq_qbyte(const uint8_t *buf, uint32_t start, uint32_t L, uint32_t qs, uint32_t qn, int32_t qmin, uint32_t i) {
  uint32_t c = buf[start + i];
  if (i < L && qmin > -128) {
    const int32_t qv = i < qn ? (int32_t)(int8_t)buf[qs + i] : 0;
    if (qv < qmin) c = (uint32_t)'N';
  }
  return c;
}

/* rows [r0, r1) of the chunk, r1 <= nrec: row r is line 4r + 1 with its '\n' (always there), quality-masked, zero-padded.  Loads:
 * the sequence line the walk found, and qinfo's [start, start + length) clamped to [t0, e1). */
__global__ void __launch_bounds__(64 * MK_FQ_WAVES) mk_fq_rows_q_kernel(const uint8_t *buf, uint32_t t0, uint32_t e1, uint32_t ntiles,
                                                                        const uint32_t *tile_base, uint32_t r0, uint32_t r1, uint32_t stride,
                                                                        const uint32_t *qinfo, int32_t qmin, uint8_t *rows) {
  __shared__ uint32_t ev_start[MK_FQ_WAVES][MK_FQ_TILE / 4], ev_len[MK_FQ_WAVES][MK_FQ_TILE / 4], ev_row[MK_FQ_WAVES][MK_FQ_TILE / 4];
  __shared__ uint32_t ev_n[MK_FQ_WAVES];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, tile = blockIdx.x * MK_FQ_WAVES + wave;
  if (tile >= ntiles) return;
  if (lane == 0u) ev_n[wave] = 0u;
  mk_lds_fence();
  mk_fq_walk(buf, t0, e1, tile, tile_base[tile], lane, [&](uint32_t j, int32_t q, uint32_t p) {
    const uint32_t r = j >> 2;
    if ((j & 3u) != 1u || r < r0 || r >= r1) return;
    const uint32_t at = atomicAdd(&ev_n[wave], 1u);
    ev_start[wave][at] = (uint32_t)(q + 1);
    ev_len[wave][at] = (uint32_t)((int32_t)p - q);
    ev_row[wave][at] = r - r0;
  });
  mk_lds_fence();
  const uint32_t n = ev_n[wave];
  for (uint32_t e = 0; e < n; e++) {
    const uint32_t start = ev_start[wave][e], row = ev_row[wave][e];
    uint32_t len = ev_len[wave][e];
    if (len > stride) len = stride; /* (cannot happen: the stride comes from the longest of these lines) */
    uint32_t qs = qinfo[2u * (r0 + row)], qn = qinfo[2u * (r0 + row) + 1u];
    if (qs < t0 || qs > e1) { qs = t0; qn = 0u; } /* (cannot happen: the reduce walk wrote both from newlines of the text) */
    if (qn > e1 - qs) qn = e1 - qs;
    const uint32_t L = len - 1u; /* len >= 1: the line's '\n' */
    uint32_t *dst = (uint32_t *)(rows + (uint64_t)row * stride);
    for (uint32_t o = 4u * lane; o < stride; o += 256u) {
      uint32_t w = 0;
      for (uint32_t k = 0; k < 4u; k++) if (o + k < len) w |= mk_fq_qbyte(buf, start, L, qs, qn, qmin, o + k) << (8u * k);
      dst[o >> 2] = w;
    }
  }
}

/* The first record of a file without a complete one (fewer than four newlines, so fewer than four lines of at most 4095 bytes: the
 * caller has checked the longest line): one wave finds the first three newlines, 64 bytes a step.  The sequence is line 2 without
 * its '\n', the quality line is line 4 if the text has one, as far as it goes.  The row goes to rows[0, MK_ROW_PITCH(L + 1)), which
 * is at most 4096 bytes; res->maxseq = L + 1 and res->nrec = 1 tell the host; a text without a second line leaves both as they are. */
__global__ void __launch_bounds__(64) mk_fq_first_q_kernel(const uint8_t *buf, uint32_t t0, uint32_t e1, int32_t qmin, mk_fq_res *res, uint8_t *rows) {
  const uint32_t lane = threadIdx.x;
  uint32_t nlp[3] = {e1, e1, e1}, found = 0;
  for (uint32_t b = t0; b < e1 && found < 3u; b += 64u) {
    uint64_t m = __ballot(b + lane < e1 && buf[b + lane] == (uint8_t)'\n');
    while (m && found < 3u) { nlp[found++] = b + (uint32_t)__builtin_ctzll(m); m &= m - 1ull; }
  }
  if (nlp[0] + 1u >= e1) return; /* no second line: no record */
  const uint32_t start = nlp[0] + 1u;
  uint32_t L = nlp[1] - start;
  if (L > MK_FQ_LINE_MAX - 1u) L = MK_FQ_LINE_MAX - 1u; /* (cannot happen, see above) */
  const uint32_t qs = nlp[2] < e1 ? nlp[2] + 1u : e1, qn = e1 - qs;
  const uint32_t stride = mk_fq_stride_dev(L + 1u);
  uint32_t *dst = (uint32_t *)rows;
  for (uint32_t o = 4u * lane; o < stride; o += 256u) {
    uint32_t w = 0;
    for (uint32_t k = 0; k < 4u; k++) {
      if (o + k < L) w |= mk_fq_qbyte(buf, start, L, qs, qn, qmin, o + k) << (8u * k);
      else if (o + k == L) w |= (uint32_t)'\n' << (8u * k);
    }
    dst[o >> 2] = w;
  }
  if (lane == 0u) { res->maxseq = L + 1u; res->nrec = 1u; }
}

/* src[from, from + n) -> dst[to, to + n): the bytes behind a chunk's last complete record, n <= MK_FQ_CARRY */
__global__ void __launch_bounds__(256) mk_fq_carry_kernel(const uint8_t *src, uint32_t from, uint8_t *dst, uint32_t to, uint32_t n) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[to + i] = src[from + i];
}

} /* namespace */

/* ---- launches, on any stream ------------------------------------------------------------------------------------------------ */
static inline uint32_t mk_fq_ntiles(uint32_t e1) { return e1 ? (e1 + MK_FQ_TILE - 1) / MK_FQ_TILE : 1u; }
/* bytes a text buffer needs for text that ends at buffer position e1: whole tiles */
static inline uint64_t mk_fq_buf_bytes(uint64_t e1) { return ((e1 + MK_FQ_TILE - 1) / MK_FQ_TILE + 1) * (uint64_t)MK_FQ_TILE; }
/* count + scan + reduce: *d_res is complete when the stream gets there */
static hipError_t mk_launch_frame_count(hipStream_t s, const uint8_t *d_buf, uint32_t t0, uint32_t e1, int final, uint32_t *d_tile_cnt, uint32_t *d_tile_last,
                                        const uint32_t *d_status, uint32_t nblocks, mk_fq_res *d_res) {
  const uint32_t nt = mk_fq_ntiles(e1), grid = (nt + MK_FQ_WAVES - 1) / MK_FQ_WAVES;
  hipLaunchKernelGGL(mk_fq_count_kernel, dim3(grid), dim3(64 * MK_FQ_WAVES), 0, s, d_buf, t0, e1, nt, d_tile_cnt, d_tile_last);
  hipLaunchKernelGGL(mk_fq_scan_kernel, dim3(1), dim3(1024), 0, s, d_tile_cnt, (const uint32_t *)d_tile_last, nt, t0, e1, final, d_status, nblocks, d_res);
  hipLaunchKernelGGL(mk_fq_reduce_kernel, dim3(grid), dim3(64 * MK_FQ_WAVES), 0, s, d_buf, t0, e1, nt, (const uint32_t *)d_tile_cnt, final, d_res);
  return hipGetLastError();
}
static hipError_t mk_launch_frame_rows(hipStream_t s, const uint8_t *d_buf, uint32_t t0, uint32_t e1, const uint32_t *d_tile_cnt, uint32_t r0, uint32_t r1,
                                       uint32_t stride, uint8_t *d_rows) {
  if (r1 <= r0) return hipSuccess;
  const uint32_t nt = mk_fq_ntiles(e1), grid = (nt + MK_FQ_WAVES - 1) / MK_FQ_WAVES;
  hipLaunchKernelGGL(mk_fq_rows_kernel, dim3(grid), dim3(64 * MK_FQ_WAVES), 0, s, d_buf, t0, e1, nt, d_tile_cnt, r0, r1, stride, d_rows);
  return hipGetLastError();
}
static inline uint32_t mk_fq_stride(uint32_t maxseq) { const uint32_t need = maxseq ? maxseq : 1u; return MK_ROW_PITCH(need); }

/* fastq2co's reader.  Records a text of n bytes can hold: four newlines each */
static inline uint32_t mk_fq_qcap(uint64_t n) { return (uint32_t)(n / 4u + 1u); }
static hipError_t mk_launch_frame_count_q(hipStream_t s, const uint8_t *d_buf, uint32_t t0, uint32_t e1, int final, uint32_t *d_tile_cnt, uint32_t *d_tile_last,
                                          const uint32_t *d_status, uint32_t nblocks, mk_fq_res *d_res, uint32_t *d_qinfo, uint32_t qcap) {
  const uint32_t nt = mk_fq_ntiles(e1), grid = (nt + MK_FQ_WAVES - 1) / MK_FQ_WAVES;
  hipLaunchKernelGGL(mk_fq_count_kernel, dim3(grid), dim3(64 * MK_FQ_WAVES), 0, s, d_buf, t0, e1, nt, d_tile_cnt, d_tile_last);
  hipLaunchKernelGGL(mk_fq_scan_kernel, dim3(1), dim3(1024), 0, s, d_tile_cnt, (const uint32_t *)d_tile_last, nt, t0, e1, 0, d_status, nblocks, d_res);
  hipLaunchKernelGGL(mk_fq_reduce_q_kernel, dim3(grid), dim3(64 * MK_FQ_WAVES), 0, s, d_buf, t0, e1, nt, (const uint32_t *)d_tile_cnt, final, d_res, d_qinfo, qcap);
  return hipGetLastError();
}
static hipError_t mk_launch_frame_rows_q(hipStream_t s, const uint8_t *d_buf, uint32_t t0, uint32_t e1, const uint32_t *d_tile_cnt, uint32_t r0, uint32_t r1,
                                         uint32_t stride, const uint32_t *d_qinfo, int32_t qmin, uint8_t *d_rows) {
  if (r1 <= r0) return hipSuccess;
  const uint32_t nt = mk_fq_ntiles(e1), grid = (nt + MK_FQ_WAVES - 1) / MK_FQ_WAVES;
  hipLaunchKernelGGL(mk_fq_rows_q_kernel, dim3(grid), dim3(64 * MK_FQ_WAVES), 0, s, d_buf, t0, e1, nt, d_tile_cnt, r0, r1, stride, d_qinfo, qmin, d_rows);
  return hipGetLastError();
}
/* what the read-back of mk_launch_frame_count_q means on the host: on a final call everything is consumed and a text without a
 * newline is one line.  Returns whether mk_fq_first_q_kernel must look at the text: a final call, no record so far, none here, and
 * a first line that ends (whether a second one follows it is the kernel's to see). */
static inline bool mk_fq_res_q(mk_fq_res &r, uint32_t n, int final, uint64_t records_before) {
  if (!final) return false;
  r.consumed = n;
  if (r.nl == 0u && n > r.maxline) r.maxline = n;
  return records_before == 0 && r.nrec == 0u && r.nl > 0u;
}

/* ---- the host side, once ------------------------------------------------------------------------------------------------------
 * One chunk of text at a time, buf[t0, e1) on the device: count() queues the count phase and the read-back and returns; result()
 * waits for it; rows() hands the chunk's rows out in portions.  What the caller queues between count() and result() runs beside the
 * count phase. */
struct mk_fq_chunk { /* what result() says about the chunk count() was given */
  mk_fq_res r;
  uint32_t stride;       /* the row pitch of r.nrec rows */
  bool first, long_line; /* the first-record exception applies (rows() runs it); a line of MK_FQ_LINE_MAX bytes, or more left over than a carry holds */
};
struct mk_fq_handed { /* what rows() did */
  uint64_t rows;          /* rows handed to push so far: up to date at every call of push */
  uint32_t stride, carry; /* their pitch (the first record's, where that was the row); bytes behind the last complete record */
  int push_rc;            /* what push returned when it ended the loop, else MK_OK */
};

#define MK_FQ_TRY(call) do { const hipError_t _e = (call); if (_e != hipSuccess) return _e; } while (0)

struct mk_fq_framer {
  bool occ = false; /* false: mk_fastq_frame's rule (-A); true: mk_fastq_frame_q's, bases below qmin masked */
  int32_t qmin = 0;
  uint32_t *d_tile_cnt = nullptr, *d_tile_last = nullptr, *d_qinfo = nullptr; /* d_qinfo: occ only, two words per record a text can hold */
  uint8_t *d_rows = nullptr;
  uint64_t tiles_cap = 0, tiles_last_cap = 0, qinfo_cap = 0, rows_cap = 0;
  uint64_t portion = 0; /* row bytes handed out at a time: the most reserve() was asked for */
  uint32_t qcap = 0;
  mk_fq_res *d_res = nullptr, *h_res = nullptr;
  hipEvent_t ev_res = nullptr, ev_t[4] = {nullptr, nullptr, nullptr, nullptr}; /* count phase: ev_t[0..1], first rows launch: ev_t[2..3] */
  bool rows_timed = false;
  const uint8_t *buf = nullptr; /* the chunk in hand */
  uint32_t t0 = 0, e1 = 0;
  int final = 0;

  ~mk_fq_framer() {
    (void)hipFree(d_tile_cnt); (void)hipFree(d_tile_last); (void)hipFree(d_qinfo); (void)hipFree(d_rows); (void)hipFree(d_res);
    if (h_res) (void)hipHostFree(h_res);
    if (ev_res) (void)hipEventDestroy(ev_res);
    for (hipEvent_t e : ev_t) if (e) (void)hipEventDestroy(e);
  }

  /* binds the mode; the first call makes the events and the result words */
  hipError_t setup(bool occ_, int32_t qmin_) {
    occ = occ_; qmin = qmin_;
    if (!d_res) MK_FQ_TRY(mk_dev_alloc(&d_res, sizeof(mk_fq_res)));
    if (!h_res) MK_FQ_TRY(mk_pin_alloc(&h_res, sizeof(mk_fq_res), hipHostMallocDefault));
    if (!ev_res) MK_FQ_TRY(hipEventCreateWithFlags(&ev_res, hipEventDisableTiming));
    for (hipEvent_t &e : ev_t) if (!e) MK_FQ_TRY(hipEventCreate(&e));
    return hipSuccess;
  }

  /* room for texts that end at buffer position text_end and for portions of row_bytes (never below MK_FQ_LINE_MAX: the first
   * record's row, whatever its stride).  Buffers only grow; one that is replaced is freed behind a wait for s, which may still use it */
  hipError_t reserve(hipStream_t s, uint64_t text_end, uint64_t row_bytes) {
    const uint64_t nt = mk_fq_ntiles((uint32_t)text_end), qneed = occ ? 2u * (uint64_t)mk_fq_qcap(text_end) : 0u;
    if (row_bytes < MK_FQ_LINE_MAX) row_bytes = MK_FQ_LINE_MAX;
    if ((d_tile_cnt && nt > tiles_cap) || (d_qinfo && qneed > qinfo_cap) || (d_rows && row_bytes > rows_cap)) MK_FQ_TRY(hipStreamSynchronize(s));
    MK_FQ_TRY(mk_grow(&d_tile_cnt, &tiles_cap, nt, false));
    MK_FQ_TRY(mk_grow(&d_tile_last, &tiles_last_cap, nt, false));
    if (occ) MK_FQ_TRY(mk_grow(&d_qinfo, &qinfo_cap, qneed, false));
    MK_FQ_TRY(mk_grow(&d_rows, &rows_cap, row_bytes, false));
    if (occ && mk_fq_qcap(text_end) > qcap) qcap = mk_fq_qcap(text_end);
    if (row_bytes > portion) portion = row_bytes;
    return hipSuccess;
  }

  /* the count phase of buf[t0, e1) in the mode's flavour and the read-back of its result, queued on s; does not wait */
  hipError_t count(hipStream_t s, const uint8_t *d_buf, uint32_t t0_, uint32_t e1_, int final_, const uint32_t *d_status, uint32_t nblocks) {
    buf = d_buf; t0 = t0_; e1 = e1_; final = final_;
    MK_FQ_TRY(hipEventRecord(ev_t[0], s));
    if (occ) MK_FQ_TRY(mk_launch_frame_count_q(s, buf, t0, e1, final, d_tile_cnt, d_tile_last, d_status, nblocks, d_res, d_qinfo, qcap));
    else MK_FQ_TRY(mk_launch_frame_count(s, buf, t0, e1, final, d_tile_cnt, d_tile_last, d_status, nblocks, d_res));
    MK_FQ_TRY(hipEventRecord(ev_t[1], s));
    MK_FQ_TRY(hipMemcpyAsync(h_res, d_res, sizeof(mk_fq_res), hipMemcpyDeviceToHost, s));
    return hipEventRecord(ev_res, s);
  }

  /* the one wait per chunk.  records_before: rows the file has given so far (occ: decides the first-record exception) */
  hipError_t result(uint64_t records_before, mk_fq_chunk *c) {
    MK_FQ_TRY(hipEventSynchronize(ev_res));
    const uint32_t n = e1 - t0;
    c->r = *h_res;
    c->first = occ && mk_fq_res_q(c->r, n, final, records_before);
    c->stride = mk_fq_stride(c->r.maxseq);
    c->long_line = c->r.maxline >= MK_FQ_LINE_MAX || (!final && n - c->r.consumed > MK_FQ_CARRY);
    return hipSuccess;
  }

  /* milliseconds of the count phase result() waited for and, once (else 0), of the first rows launch of the rows() before it;
   * behind a wait for the stream that is the last rows()'s */
  hipError_t times(float *count_ms, float *rows_ms) {
    *rows_ms = 0.f;
    if (rows_timed) MK_FQ_TRY(hipEventElapsedTime(rows_ms, ev_t[2], ev_t[3]));
    rows_timed = false;
    return hipEventElapsedTime(count_ms, ev_t[0], ev_t[1]);
  }

  /* the chunk's rows: the first record's where c.first says so (a file without a complete record: its first one is walked all the
   * same, if it has a sequence line), then r.nrec rows in portions.  push(d_rows, stride, nrows) -> MK_OK, or what ends the loop */
  template <class Push>
  hipError_t rows(hipStream_t s, const mk_fq_chunk &c, Push push, mk_fq_handed *out) {
    *out = mk_fq_handed{0, c.stride, (e1 - t0) - c.r.consumed, MK_OK};
    if (c.first) {
      hipLaunchKernelGGL(mk_fq_first_q_kernel, dim3(1), dim3(64), 0, s, buf, t0, e1, qmin, d_res, d_rows);
      MK_FQ_TRY(hipGetLastError());
      MK_FQ_TRY(hipMemcpyAsync(h_res, d_res, sizeof(mk_fq_res), hipMemcpyDeviceToHost, s));
      MK_FQ_TRY(hipStreamSynchronize(s));
      if (h_res->nrec) {
        out->stride = mk_fq_stride(h_res->maxseq);
        if ((out->push_rc = push(d_rows, out->stride, 1u)) != MK_OK) return hipSuccess;
        out->rows = 1;
      }
    }
    const uint32_t per = (uint32_t)(portion / c.stride);
    if (c.r.nrec) MK_FQ_TRY(hipEventRecord(ev_t[2], s));
    for (uint32_t r0 = 0; r0 < c.r.nrec; r0 += per) {
      const uint32_t r1 = c.r.nrec - r0 < per ? c.r.nrec : r0 + per;
      if (occ) MK_FQ_TRY(mk_launch_frame_rows_q(s, buf, t0, e1, d_tile_cnt, r0, r1, c.stride, d_qinfo, qmin, d_rows));
      else MK_FQ_TRY(mk_launch_frame_rows(s, buf, t0, e1, d_tile_cnt, r0, r1, c.stride, d_rows));
      if (r0 == 0) { MK_FQ_TRY(hipEventRecord(ev_t[3], s)); rows_timed = true; }
      if ((out->push_rc = push(d_rows, c.stride, r1 - r0)) != MK_OK) return hipSuccess;
      out->rows += r1 - r0;
    }
    return hipSuccess;
  }
};
