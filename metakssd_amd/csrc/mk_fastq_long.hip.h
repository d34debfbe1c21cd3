/*
 * mk_fastq_long.hip.h -- device side of mk_sketch_push_fastq_long(): FASTQ text of any line length -> base stream (gfx950, wave64).
 *
 * mt_shortreads2koc() (iseq2comem.c:672-720) takes four fgets() lines a record and walks the second one up to its '\n'; a byte that
 * is no base resets the k-mer window (:682-690).  Its FQ_LEN (:656) cuts lines of 4 095 characters and more and mis-frames the file
 * from there on; this route is the same loop with FQ_LEN unbounded.  It is the FASTQ flavour of mk_stream.hip.h -- the same three
 * kernels with another rule for which bytes stay:
 *     role of a byte : (number of '\n' in front of it) mod 4 -- 0 header, 1 sequence, 2 '+' line, 3 quality
 *     kept           : exactly the bytes of role 1, whatever they are ('\r', 'N', bytes >= 0x80: the scan kernel resets on them as the
 *                      reference's loop does); the '\n' that ends the line goes in as ONE '>' (no base and no row end: the window
 *                      resets between two reads, as `base = 1` does at the top of the per-read loop)
 *     dropped        : every byte of the other three lines, whatever it is
 * The state is a newline count, so a segment's summary is {its newlines, bytes kept for each of the four entry roles}, and composing
 * the summaries is two plain prefix sums: newlines (-> entry role of every segment), then the kept bytes for that role.
 *
 * Record rule (:673): a record counts when its fourth fgets() gives at least one byte.  The text of one push always starts at a record
 * start (the engine puts the open record in front of the next push's text, mk_engine.hip), so with N newlines in the push the last
 * record ends behind newline number 4 * (N / 4); the scan kernel finds that byte (`consumed`), the emit kernel stops there.  The
 * final push also takes a last record whose quality line has bytes but no '\n' (N mod 4 == 3, last byte no '\n').
 *   mk_fql_summary_kernel  one wave per segment of MK_FA_SEG bytes
 *   mk_fql_scan_kernel     one workgroup: prefix sums, the cut, stream length and row count (as mk_fa_scan_kernel)
 *   mk_fql_emit_kernel     the same walk with the entry role known: kept bytes to stream[offset ..], up to the cut
 *   mk_fql_carry_kernel    the text behind the cut (the open record) to the engine's carry buffer: it never leaves HBM
 *
 * The quality-aware flavour (mk_sketch_push_fastq_long_q) is fastq2co()'s reader (iseq2comem.c:343-379) with its
 * fgets() width unbounded: the same roles and the same stream bytes, but a base whose quality byte (signed) is below qmin goes in as
 * 'N', a record counts only when all four of its lines end in '\n', and the first record of a file is walked whenever its second
 * line exists (mk_fastq_frame_q's rule).  The stream is written from the QUALITY line: the lane that holds column c of a record's
 * fourth line loads the base from column c of its second line -- whose place it knows from the last three newlines in front of it --
 * and stores base or 'N'; no lane of a sequence line stores anything, so every stream byte has one writer.
 *   mk_fqq_summary_kernel  mk_fql_summary_kernel + the segment's own last three newline offsets (mk_fqq_nl)
 *   mk_fqq_scan_kernel     mk_fql_scan_kernel without the open-end exception + the last three newlines in front of every segment
 *   mk_fqq_emit_kernel     the walk driven by the role-3 bytes
 *   mk_fqq_first_kernel    the first-record exception of the final push: no record counted, the text's second line masked and kept
 */
#pragma once
#include "mk_stream.hip.h"

struct mk_fql_sum { /* per segment */
  uint32_t cnt[4]; /* bytes kept when the segment is entered in role 0..3 */
  uint32_t nl;     /* newlines in the segment */
  uint32_t nlpre;  /* scan: newlines in front of the segment (its entry role is nlpre & 3) */
  uint32_t off;    /* scan: output offset of the segment, relative to the stream length before this push */
  uint32_t pad;
};

/* the quality-aware flavour: the most recent newlines, at most three -- k of them, p[0] the nearest; text offsets (a push is below 2^31
 * bytes).  Joining `a` in front of `b` keeps b's and fills up with a's nearest: a shift register three deep, associative. */
struct mk_fqq_nl {
  uint32_t k;
  uint32_t p[3];
};

__device__ __forceinline__ mk_fqq_nl mk_fqq_join(const mk_fqq_nl &a, const mk_fqq_nl &b) {
  mk_fqq_nl r;
  const uint32_t k = b.k;
  r.p[0] = k >= 1u ? b.p[0] : a.p[0];
  r.p[1] = k >= 2u ? b.p[1] : (k == 1u ? a.p[0] : a.p[1]);
  r.p[2] = k >= 3u ? b.p[2] : (k == 2u ? a.p[0] : (k == 1u ? a.p[1] : a.p[2]));
  r.k = a.k + k < 3u ? a.k + k : 3u;
  return r;
}

/* the three highest bits of a step's newline mask as offsets from `base` */
__device__ __forceinline__ mk_fqq_nl mk_fqq_top3(uint64_t m, uint32_t base) {
  mk_fqq_nl r = {0u, {0u, 0u, 0u}};
#pragma unroll
  for (uint32_t t = 0; t < 3u; t++) {
    if (m) {
      const uint32_t at = 63u - (uint32_t)__builtin_clzll(m);
      r.p[t] = base + at;
      r.k = t + 1u;
      m ^= 1ull << at;
    }
  }
  return r;
}

/* one 64-byte step entered in role `role` (wave-uniform): the lanes whose bytes are kept; role := the role behind the step */
__device__ __forceinline__ uint64_t mk_fql_step(uint8_t ch, bool valid, uint32_t lane, uint32_t &role) {
  const uint64_t nl = __ballot(valid && ch == '\n');
  if (nl == 0ull) return role == 1u ? __ballot(valid) : 0ull; /* inside one line: nearly every step of a long read */
  const uint64_t below = lane ? (~0ull >> (64u - lane)) : 0ull; /* lanes in front of this one */
  const uint32_t mine = (role + (uint32_t)__popcll(nl & below)) & 3u;
  role = (role + (uint32_t)__popcll(nl)) & 3u;
  return __ballot(valid && mine == 1u);
}

/* Q: also the segment's own last three newlines to last[segi] */
template <bool Q>
__device__ __forceinline__ void mk_fql_summary_body(const uint8_t *text, uint64_t n, mk_fql_sum *sum, mk_fqq_nl *last) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t segi = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t lo = segi * MK_FA_SEG;
  if (lo >= n) return;
  const uint64_t hi = lo + MK_FA_SEG < n ? lo + MK_FA_SEG : n;
  __shared__ uint4 seg_lds[MK_FA_WAVES][64];
  const uint8_t *seg = mk_fa_stage(text, lo, lane, seg_lds[threadIdx.x >> 6]);
  const uint32_t len = (uint32_t)(hi - lo);
  const uint64_t below = lane ? (~0ull >> (64u - lane)) : 0ull;
  uint32_t c[4] = {0u, 0u, 0u, 0u}, nls = 0u;
  mk_fqq_nl l3 = {0u, {0u, 0u, 0u}};
#pragma unroll
  for (uint32_t j = 0; j < MK_FA_SEG / 64u; j++) {
    if (64u * j >= len) break;
    const bool valid = 64u * j + lane < len;
    const uint8_t ch = seg[64u * j + lane];
    const uint64_t nl = __ballot(valid && ch == '\n');
    /* q: newlines of the segment in front of this byte, mod 4; entered in role r the byte has role (r + q) & 3, kept when that is 1 */
    const uint32_t q = (nls + (uint32_t)__popcll(nl & below)) & 3u;
    if (nl == 0ull) { /* one line: q is the same in every lane */
      const uint32_t all = (uint32_t)__popcll(__ballot(valid));
#pragma unroll
      for (uint32_t r = 0; r < 4u; r++) c[r] += ((r + q) & 3u) == 1u ? all : 0u;
    } else {
#pragma unroll
      for (uint32_t r = 0; r < 4u; r++) c[r] += (uint32_t)__popcll(__ballot(valid && ((r + q) & 3u) == 1u));
    }
    nls += (uint32_t)__popcll(nl);
    if (Q && nl) l3 = mk_fqq_join(l3, mk_fqq_top3(nl, (uint32_t)lo + 64u * j));
  }
  if (lane == 0) {
    mk_fql_sum r;
    r.cnt[0] = c[0]; r.cnt[1] = c[1]; r.cnt[2] = c[2]; r.cnt[3] = c[3];
    r.nl = nls; r.nlpre = 0u; r.off = 0u; r.pad = 0u;
    sum[segi] = r;
    if (Q) last[segi] = l3;
  }
}

__global__ void __launch_bounds__(256) mk_fql_summary_kernel(const uint8_t *text, uint64_t n, mk_fql_sum *sum) {
  mk_fql_summary_body<false>(text, n, sum, nullptr);
}

__global__ void __launch_bounds__(256) mk_fqq_summary_kernel(const uint8_t *text, uint64_t n, mk_fql_sum *sum, mk_fqq_nl *last) {
  mk_fql_summary_body<true>(text, n, sum, last);
}

/* exclusive prefix sum over the workgroup's 1024 threads (all of them call); total := the sum of all */
__device__ __forceinline__ uint32_t mk_fql_block_scan(uint32_t v, uint32_t &total) {
  __shared__ uint32_t wsum[16];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (uint32_t o = 1; o < 64u; o <<= 1) {
    const uint32_t p = __shfl_up(inc, o);
    if (lane >= o) inc += p;
  }
  __syncthreads(); /* (the call before this one has been read) */
  if (lane == 63u) wsum[wave] = inc;
  __syncthreads();
  uint32_t base = 0u, all = 0u;
  for (uint32_t w = 0; w < 16u; w++) { if (w < wave) base += wsum[w]; all += wsum[w]; }
  total = all;
  return base + inc - v;
}

__device__ __forceinline__ mk_fqq_nl mk_fqq_shfl_up(const mk_fqq_nl &v, uint32_t o) {
  mk_fqq_nl r;
  r.k = __shfl_up(v.k, o);
  r.p[0] = __shfl_up(v.p[0], o); r.p[1] = __shfl_up(v.p[1], o); r.p[2] = __shfl_up(v.p[2], o);
  return r;
}

/* the same for mk_fqq_join: what the threads in front of this one give, joined in thread order; total := all of them */
__device__ __forceinline__ mk_fqq_nl mk_fqq_block_scan(const mk_fqq_nl &v, mk_fqq_nl &total) {
  __shared__ mk_fqq_nl wl[16];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const mk_fqq_nl none = {0u, {0u, 0u, 0u}};
  mk_fqq_nl inc = v;
#pragma unroll
  for (uint32_t o = 1; o < 64u; o <<= 1) {
    const mk_fqq_nl p = mk_fqq_shfl_up(inc, o);
    if (lane >= o) inc = mk_fqq_join(p, inc);
  }
  mk_fqq_nl ex = mk_fqq_shfl_up(inc, 1u);
  if (lane == 0u) ex = none;
  __syncthreads(); /* (the call before this one has been read) */
  if (lane == 63u) wl[wave] = inc;
  __syncthreads();
  mk_fqq_nl base = none, all = none;
  for (uint32_t w = 0; w < 16u; w++) { if (w < wave) base = mk_fqq_join(base, wl[w]); all = mk_fqq_join(all, wl[w]); }
  total = all;
  return mk_fqq_join(base, ex);
}

/* One workgroup of 1024 threads.  The push's text starts at a record start (role 0).  st->in_header := `consumed`, the text offset
 * behind the last byte of the last complete record (0: none); st->len, st->nrows as mk_fa_scan_kernel sets them, for the kept bytes
 * in front of that offset only.
 * Q: fastq2co's record rule -- no record without its fourth '\n' -- and last[i] := the last three newlines in front of segment i
 * (from its own, as mk_fqq_summary_kernel left them), last[nseg] := those of the whole text. */
template <bool Q>
__device__ __forceinline__ void mk_fql_scan_body(mk_fql_sum *sum, uint64_t nseg, const uint8_t *text, uint64_t n, mk_fa_state *st, uint8_t *stream,
                                                 uint32_t pitch, uint32_t rowlen, uint32_t TL, int final, mk_fqq_nl *last) {
  __shared__ uint32_t cut_seg, cut_pos, cut_kept;
  __shared__ uint4 seg_lds[64];
  /* newlines in front of every segment */
  uint32_t carry = 0u;
  for (uint64_t base = 0; base < nseg; base += 1024u) {
    const uint64_t i = base + threadIdx.x;
    uint32_t total;
    const uint32_t ex = mk_fql_block_scan(i < nseg ? sum[i].nl : 0u, total);
    if (i < nseg) sum[i].nlpre = carry + ex;
    carry += total;
  }
  const uint32_t N = carry;
  /* the last record: ends behind newline number want (counted from 1), or with the text */
  const bool open_end = !Q && final && n && (N & 3u) == 3u && text[n - 1] != (uint8_t)'\n';
  const uint32_t want = N & ~3u;
  if (threadIdx.x == 0) { cut_seg = 0xFFFFFFFFu; cut_pos = 0u; cut_kept = 0u; }
  __syncthreads();
  /* output offset of every segment; the segment that holds the cut */
  carry = 0u;
  for (uint64_t base = 0; base < nseg; base += 1024u) {
    const uint64_t i = base + threadIdx.x;
    uint32_t mine = 0u, pre = 0u, nl = 0u;
    if (i < nseg) { pre = sum[i].nlpre; nl = sum[i].nl; mine = sum[i].cnt[pre & 3u]; }
    uint32_t total;
    const uint32_t ex = mk_fql_block_scan(mine, total);
    if (i < nseg) {
      sum[i].off = carry + ex;
      if (!open_end && want && pre < want && want <= pre + nl) cut_seg = (uint32_t)i; /* exactly one segment */
    }
    carry += total;
  }
  const uint32_t K = carry;
  __syncthreads();
  /* one wave walks that segment up to its newline number want - nlpre: where it is, and what is kept up to and with it */
  if (threadIdx.x < 64u && cut_seg != 0xFFFFFFFFu) {
    const uint32_t lane = threadIdx.x;
    const uint64_t lo = (uint64_t)cut_seg * MK_FA_SEG;
    const uint32_t len = (uint32_t)(lo + MK_FA_SEG < n ? MK_FA_SEG : n - lo);
    uint32_t left = want - sum[cut_seg].nlpre; /* newlines still to pass, the wanted one included */
    uint32_t role = sum[cut_seg].nlpre & 3u, kept = 0u;
    const uint8_t *seg = mk_fa_stage(text, lo, lane, seg_lds);
    for (uint32_t j = 0; j < MK_FA_SEG / 64u; j++) {
      if (64u * j >= len) break;
      const bool valid = 64u * j + lane < len;
      const uint8_t ch = seg[64u * j + lane];
      uint64_t nl = __ballot(valid && ch == '\n');
      const uint64_t keep = mk_fql_step(ch, valid, lane, role);
      const uint32_t here = (uint32_t)__popcll(nl);
      if (here < left) { left -= here; kept += (uint32_t)__popcll(keep); continue; }
      for (uint32_t t = 1; t < left; t++) nl &= nl - 1ull; /* drop the newlines in front of the wanted one */
      const uint32_t at = (uint32_t)__builtin_ctzll(nl);
      kept += (uint32_t)__popcll(keep & ((2ull << at) - 1ull));
      if (lane == 0) { cut_pos = 64u * j + at + 1u; cut_kept = kept; }
      break;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long consumed = 0ull, kept = 0ull;
    if (open_end) { consumed = n; kept = K; }
    else if (cut_seg != 0xFFFFFFFFu) { consumed = (unsigned long long)cut_seg * MK_FA_SEG + cut_pos; kept = (unsigned long long)sum[cut_seg].off + cut_kept; }
    const unsigned long long len = st->len + kept;
    st->len = len;
    st->in_header = (uint32_t)consumed;
    unsigned long long rows = 0;
    if (final) {
      if (len >= TL) rows = (len - (TL - 1u) + pitch - 1u) / pitch; /* every row with a complete k-mer in it */
      stream[len] = (uint8_t)'\n'; /* the last row ends here */
    } else if (len >= rowlen) rows = (len - rowlen) / pitch + 1u; /* complete rows only */
    st->nrows = rows;
  }
  if (Q) {
    mk_fqq_nl front = {0u, {0u, 0u, 0u}};
    for (uint64_t base = 0; base < nseg; base += 1024u) {
      const uint64_t i = base + threadIdx.x;
      mk_fqq_nl mine = {0u, {0u, 0u, 0u}}, total;
      if (i < nseg) mine = last[i];
      const mk_fqq_nl ex = mk_fqq_block_scan(mine, total);
      if (i < nseg) last[i] = mk_fqq_join(front, ex);
      front = mk_fqq_join(front, total);
    }
    if (threadIdx.x == 0) last[nseg] = front;
  }
}

__global__ void __launch_bounds__(1024) mk_fql_scan_kernel(mk_fql_sum *sum, uint64_t nseg, const uint8_t *text, uint64_t n, mk_fa_state *st,
                                                          uint8_t *stream, uint32_t pitch, uint32_t rowlen, uint32_t TL, int final) {
  mk_fql_scan_body<false>(sum, nseg, text, n, st, stream, pitch, rowlen, TL, final, nullptr);
}

__global__ void __launch_bounds__(1024) mk_fqq_scan_kernel(mk_fql_sum *sum, uint64_t nseg, const uint8_t *text, uint64_t n, mk_fa_state *st,
                                                          uint8_t *stream, uint32_t pitch, uint32_t rowlen, uint32_t TL, int final, mk_fqq_nl *last) {
  mk_fql_scan_body<true>(sum, nseg, text, n, st, stream, pitch, rowlen, TL, final, last);
}

/* the text once more with every segment's entry role and offset known: bytes of sequence lines in front of the cut go to the stream */
__global__ void __launch_bounds__(256) mk_fql_emit_kernel(const uint8_t *text, const mk_fql_sum *sum, const mk_fa_state *st, uint8_t *stream,
                                                         unsigned long long stream_len_before) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t segi = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t lo = segi * MK_FA_SEG, n = st->in_header; /* (this push's `consumed`: mk_fql_scan_kernel ran in front of this kernel) */
  if (lo >= n) return;
  const uint64_t hi = lo + MK_FA_SEG < n ? lo + MK_FA_SEG : n;
  __shared__ uint4 seg_lds[MK_FA_WAVES][64];
  const uint8_t *seg = mk_fa_stage(text, lo, lane, seg_lds[threadIdx.x >> 6]);
  const uint32_t len = (uint32_t)(hi - lo);
  uint32_t role = sum[segi].nlpre & 3u;
  uint64_t off = stream_len_before + sum[segi].off;
#pragma unroll
  for (uint32_t j = 0; j < MK_FA_SEG / 64u; j++) {
    if (64u * j >= len) break;
    const bool valid = 64u * j + lane < len;
    const uint8_t ch = seg[64u * j + lane];
    const uint64_t keep = mk_fql_step(ch, valid, lane, role);
    if ((keep >> lane) & 1ull) stream[off + mk_mbcnt(keep)] = ch == (uint8_t)'\n' ? (uint8_t)'>' : ch;
    off += (uint64_t)__popcll(keep);
  }
}

/* The quality-aware walk.  Every byte of role 3 in front of the cut belongs to a complete record of this text (the text starts at a
 * record start), so the three newlines in front of it exist: n1 < n2 < n3 < its own offset t.  The record's sequence line is
 * text[n1 + 1, n2), its column is c = t - (n3 + 1), and `off` at this byte -- the kept bytes in front of it -- lies just behind the
 * record's separator, so the record's stream bytes start at off - (L + 1) with L = n2 - n1 - 1.
 *   loads : text[n1 + 1 + c] with c < L, below n2 < t < consumed <= total
 *   stores: stream[record start + c], c < L, and the '>' at + L: bytes of a record in front of `consumed`, which mk_fqq_scan_kernel
 *           has counted into st->len
 * The lane of the quality line's '\n' stores the '>'; when that line is shorter than the sequence line its wave finishes the columns
 * from there on ('\n' itself is the quality of its own column, 0 stands behind it: mk_fastq_frame_q). */
__global__ void __launch_bounds__(256) mk_fqq_emit_kernel(const uint8_t *text, const mk_fql_sum *sum, const mk_fqq_nl *last, const mk_fa_state *st,
                                                         uint8_t *stream, unsigned long long stream_len_before, int32_t qmin) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t segi = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t lo = segi * MK_FA_SEG, n = st->in_header; /* (this push's `consumed`: mk_fqq_scan_kernel ran in front of this kernel) */
  if (lo >= n) return;
  const uint64_t hi = lo + MK_FA_SEG < n ? lo + MK_FA_SEG : n;
  __shared__ uint4 seg_lds[MK_FA_WAVES][64];
  const uint8_t *seg = mk_fa_stage(text, lo, lane, seg_lds[threadIdx.x >> 6]);
  const uint32_t len = (uint32_t)(hi - lo);
  const uint64_t below = lane ? (~0ull >> (64u - lane)) : 0ull;
  uint32_t role = sum[segi].nlpre & 3u;
  uint64_t off = stream_len_before + sum[segi].off;
  mk_fqq_nl front = last[segi]; /* wave-uniform: the newlines in front of the step */
#pragma unroll 1
  for (uint32_t j = 0; j < MK_FA_SEG / 64u; j++) {
    if (64u * j >= len) break;
    const bool valid = 64u * j + lane < len;
    const uint8_t ch = seg[64u * j + lane];
    const uint32_t at = (uint32_t)lo + 64u * j; /* text offset of the step */
    const uint64_t nl = __ballot(valid && ch == '\n');
    const uint32_t mine = (role + (uint32_t)__popcll(nl & below)) & 3u;
    const uint64_t keep = nl || role == 1u ? __ballot(valid && mine == 1u) : 0ull; /* what mk_fql_step keeps: counted, not stored */
    const bool isq = valid && mine == 3u;
    if (__ballot(isq)) {
      const mk_fqq_nl m = nl ? mk_fqq_join(front, mk_fqq_top3(nl & below, at)) : front;
      const uint32_t seq = m.p[2] + 1u, L = m.p[1] - seq, c = at + lane - (m.p[0] + 1u);
      const uint64_t rec = off + mk_mbcnt(keep) - ((uint64_t)L + 1u);
      const bool end = isq && ch == (uint8_t)'\n';
      if (isq && !end && c < L) stream[rec + c] = (int32_t)(int8_t)ch >= qmin ? text[seq + c] : (uint8_t)'N';
      if (end) stream[rec + L] = (uint8_t)'>';
      uint64_t rest = __ballot(end && c < L); /* quality lines shorter than their sequence lines: dirty text only */
      while (rest) {
        const int src = (int)__builtin_ctzll(rest);
        rest &= rest - 1ull;
        const uint32_t s_seq = __shfl(seq, src), s_L = __shfl(L, src), s_c = __shfl(c, src);
        const uint64_t s_rec = (uint64_t)__shfl((uint32_t)(rec >> 32), src) << 32 | __shfl((uint32_t)rec, src);
        for (uint32_t col = s_c + lane; col < s_L; col += 64u)
          stream[s_rec + col] = (col == s_c ? 10 : 0) >= qmin ? text[s_seq + col] : (uint8_t)'N';
      }
    }
    off += (uint64_t)__popcll(keep);
    if (nl) {
      role = (role + (uint32_t)__popcll(nl)) & 3u;
      front = mk_fqq_join(front, mk_fqq_top3(nl, at));
    }
  }
}

/* The first-record exception, queued behind mk_fqq_scan_kernel of a FINAL push when no earlier push of the sketch gave a record.  It
 * acts only when this push gave none either (st->in_header == 0: fewer than four newlines in the whole text, so tot = last[nseg] holds
 * all of them) and the text has a second line: that line, up to its '\n' or the end of the text, is masked by the fourth line as far
 * as that exists (0 behind it) and becomes the stream (mk_fastq_frame_q with records_before == 0).  The stream is empty up to then.
 *   loads : text[n1 + 1 + c] and text[n3 + 1 + c] below n
 *   stores: stream[before + c] for c < L <= n, and the closing '\n' at before + L; the stream buffer holds the text and a row more
 * Thread 0 alone rewrites st->len / st->nrows; no thread of this kernel reads them. */
__global__ void __launch_bounds__(256) mk_fqq_first_kernel(const uint8_t *text, uint64_t n, const mk_fqq_nl *tot, mk_fa_state *st, uint8_t *stream,
                                                          unsigned long long stream_len_before, uint32_t pitch, uint32_t TL, int32_t qmin) {
  if (st->in_header != 0u) return;
  const mk_fqq_nl t = *tot;
  if (t.k == 0u) return;
  const uint64_t s = (uint64_t)t.p[t.k - 1u] + 1u;
  if (s >= n) return; /* one line */
  const uint64_t e = t.k >= 2u ? t.p[t.k - 2u] : n, L = e - s;
  uint64_t qs = 0, qn = 0;
  if (t.k == 3u && (uint64_t)t.p[0] + 1u < n) { qs = (uint64_t)t.p[0] + 1u; qn = n - qs; }
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (uint64_t c = tid; c < L; c += (uint64_t)gridDim.x * blockDim.x) {
    const int32_t q = c < qn ? (int32_t)(int8_t)text[qs + c] : 0;
    stream[stream_len_before + c] = q >= qmin ? text[s + c] : (uint8_t)'N';
  }
  if (tid == 0) {
    const unsigned long long len = stream_len_before + L;
    st->len = len;
    st->nrows = len >= TL ? (len - (TL - 1u) + pitch - 1u) / pitch : 0ull;
    stream[len] = (uint8_t)'\n';
  }
}

/* The open record stays in HBM: text[consumed, total) -> carry[0, total - consumed), with consumed = st->in_header as mk_fql_scan_kernel
 * left it (queued behind mk_fql_emit_kernel, in front of the next push's scan kernel, the only thing that rewrites that word).  `carry`
 * is a buffer of its own: the carry is longer than `consumed` as soon as a record spans three pushes, and a move to the front of `text`
 * would then read what other threads have overwritten.  The source starts anywhere, the destination is aligned: a thread gives one
 * 16-byte store from two aligned 16-byte loads, the second only where it starts in front of `total` (whole 16-byte pieces of the text
 * buffer up to there exist: it is allocated in whole segments); carry holds total + 16 bytes at least.  A fixed grid and a stride: the
 * carry is one record as a rule. */
__global__ void __launch_bounds__(256) mk_fql_carry_kernel(const uint8_t *text, uint64_t total, const mk_fa_state *st, uint8_t *carry) {
  const uint64_t consumed = st->in_header;
  if (consumed >= total) return;
  const uint64_t base = consumed & ~(uint64_t)15u, nvec = (total - consumed + 15u) >> 4;
  const uint32_t s = (uint32_t)(consumed & 15u), r = 8u * (s & 7u);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t at = base + 16u * i;
    const uint4 a = *(const uint4 *)(text + at);
    uint4 b = make_uint4(0u, 0u, 0u, 0u);
    if (s && at + 16u < total) b = *(const uint4 *)(text + at + 16u);
    uint64_t v0 = (uint64_t)a.y << 32 | a.x, v1 = (uint64_t)a.w << 32 | a.z, v2 = (uint64_t)b.y << 32 | b.x;
    const uint64_t v3 = (uint64_t)b.w << 32 | b.z;
    if (s >= 8u) { v0 = v1; v1 = v2; v2 = v3; }
    const uint64_t o0 = r ? v0 >> r | v1 << (64u - r) : v0, o1 = r ? v1 >> r | v2 << (64u - r) : v1;
    *(uint4 *)(carry + 16u * i) = make_uint4((uint32_t)o0, (uint32_t)(o0 >> 32), (uint32_t)o1, (uint32_t)(o1 >> 32));
  }
}
