/*
 * mk_inflate.hip -- BGZF-compressed FASTQ on the device (gfx950, wave64, hand-written): inflate, CRC32, FASTQ framing.
 *
 * The reference reads a compressed input through one `zcat -fc` child (iseq2comem.c:666-669): one CPU core running inflate bounds
 * the whole path.  A BGZF file (`bgzip`) is a chain of independent gzip members of at most 64 KiB of text, each with its compressed
 * size in its header and its text size in its trailer (host/mk_bgzf.c walks them), so only the compressed bytes cross PCIe and:
 *
 *   mk_inflate_kernel    one WAVEFRONT per member, four to a workgroup.  Symbol decoding is serial per member and is done
 *                        wave-uniformly: every lane holds the same bit buffer and takes the same branches, table look-ups are LDS
 *                        broadcasts.  The compressed bytes pass through a 1 KiB window per wave in LDS, refilled by all 64 lanes (one
 *                        16-byte load each).  Code tables are built in LDS per deflate block: lane l counts and places the symbols of
 *                        length l (a canonical code is sorted by length, then symbol) and fills their entries of a 10-bit (literal /
 *                        length) or 8-bit (distance) look-up table; longer codes take the canonical bit-by-bit walk.  Literals collect
 *                        in one register (lane i holds the i-th pending literal) and leave as one store; a match is copied by all
 *                        lanes, out[pos + i] = out[pos - dist + i mod dist], which is what a byte-serial copy gives for dist < len.  A
 *                        match whose source was written since the wave last waited for its stores waits first.  Then the text's
 *                        CRC32: every lane runs the byte table over an equal slice (the text is thought padded with zero bytes IN
 *                        FRONT, which a zero register ignores; the all-ones start value is the first four bytes complemented), and
 *                        the 64 registers are folded with the 32x32 GF(2) matrix "advance by one slice", squared at every level.
 *                        Safety: loads stay inside the member's payload rounded to 16 bytes, stores inside the ISIZE bytes at the
 *                        member's offset, every loop consumes input bits or produces output bytes and is bounded by the two sizes;
 *                        malformed data ends the member with a status (MK_INFL_*), written with an ordinary store.
 * mk_fq_frame.hip.h (included behind the kernels): the FASTQ framing of text in HBM -- mk_fq_* kernels for both readers' rules and
 *                        mk_fq_framer, the host-side sequence the BGZF route, the gunzip route and the test entry points all run.
 * mk_gunzip.hip.h (included last): ONE gzip member of any size by many waves -- block-start finder, decode to 16-bit symbols with
 *                        markers, window chain, resolve -- around this file's bit reader, table builder and CRC kernels.
 * mk_gunzip_batch.hip.h (behind it): a BATCH of gzip genome files, many waves per file, as one launch sequence without a host wait:
 *                        the same finder and decode per (file, span), the piece table and the text offsets made on the device (4.16).
 * The long sinks (mk_sketch_push_bgzf_long here, mk_sketch_push_gzip_long in mk_gunzip.hip.h) reuse the inflate side of
 *                        both routes and hand the text to mk_sketch_push_fastq_long_device instead of the framer; mk_bgzf_bad_kernel
 *                        reduces a chunk's member statuses where the framer's scan kernel did.
 * Bound of each kernel: DESIGN.md 4.10, 4.12.
 */
#include <hip/hip_runtime.h>
#include "mk_poison.hip.h"

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>
#include <time.h>
#include <unistd.h>

#include "metakssd_hip.h"
#include "mk_gz.hip.h"

#define MK_INFL_WAVES 4u
#define MK_INFL_WIN 1024u      /* bytes of the compressed stream a wave holds in LDS */
#define MK_INFL_LBITS 10u
#define MK_INFL_DBITS 8u

namespace {

__device__ __forceinline__ void mk_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
/* the wave's stores to global memory are done before anything that follows is issued */
__device__ __forceinline__ void mk_store_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
__device__ __forceinline__ uint32_t mk_uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

__device__ const uint16_t mk_lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__device__ const uint8_t mk_lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__device__ const uint16_t mk_dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__device__ const uint8_t mk_dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__device__ const uint8_t mk_clorder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct mk_infl_lds { /* one wave's */
  uint32_t win[MK_INFL_WIN / 4];
  uint16_t lit_tab[1u << MK_INFL_LBITS];
  uint16_t dist_tab[1u << MK_INFL_DBITS];
  uint16_t lit_sym[288], dist_sym[32];
  uint16_t lit_cnt[16], dist_cnt[16];
  uint8_t lens[352]; /* [0, 320): literal/length + distance code lengths; [320, 339): the code length code's */
  uint32_t mat[32];
};

/* the compressed stream of one member, in coordinates relative to its payload's address rounded down to 16 bytes.  ZERO_TAIL: the
 * bytes behind `end` read as zeros whatever lies there (mk_gunzip.hip.h: a status then depends on the stream alone) */
template <bool ZERO_TAIL>
struct mk_bits_t {
  const uint8_t *base; /* 16-byte aligned */
  uint32_t *win;
  uint32_t end;        /* first byte behind the payload */
  uint32_t win_base, next, cnt;
  uint64_t buf;
  uint32_t lane;

  __device__ __forceinline__ void stage() {
    const uint32_t a = win_base + 16u * lane;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (a < end) v = *(const uint4 *)(base + a); /* (a 16-byte piece that starts inside the payload: inside the staging buffer, which ends in slack) */
    if (ZERO_TAIL && a < end && end - a < 16u) {
      const uint32_t n = end - a; /* bytes to keep */
      v.x &= n >= 4u ? ~0u : (1u << (8u * n)) - 1u;
      v.y &= n >= 8u ? ~0u : n > 4u ? (1u << (8u * (n - 4u))) - 1u : 0u;
      v.z &= n >= 12u ? ~0u : n > 8u ? (1u << (8u * (n - 8u))) - 1u : 0u;
      v.w &= n > 12u ? (1u << (8u * (n - 12u))) - 1u : 0u;
    }
    mk_lds_fence();
    ((uint4 *)win)[lane] = v;
    mk_lds_fence();
  }
  __device__ __forceinline__ void seek(uint32_t a0) {
    win_base = a0 & ~(MK_INFL_WIN - 1u);
    stage();
    const uint32_t w = mk_uni(win[(a0 & (MK_INFL_WIN - 1u)) >> 2]);
    const uint32_t sh = 8u * (a0 & 3u);
    buf = (uint64_t)(w >> sh);
    cnt = 32u - sh;
    next = (a0 & ~3u) + 4u;
  }
  /* at least 32 bits are in the buffer afterwards (zeros behind the payload's end: bitpos() tells) */
  __device__ __forceinline__ void refill() {
    if (cnt <= 32u) {
      if (next - win_base == MK_INFL_WIN) { win_base = next; stage(); }
      const uint32_t w = mk_uni(win[(next - win_base) >> 2]);
      buf |= (uint64_t)w << cnt;
      cnt += 32u;
      next += 4u;
    }
  }
  __device__ __forceinline__ uint32_t get(uint32_t n) {
    const uint32_t v = (uint32_t)buf & ((1u << n) - 1u);
    buf >>= n;
    cnt -= n;
    return v;
  }
  __device__ __forceinline__ uint64_t bitpos() const { return (uint64_t)next * 8u - cnt; }
  __device__ __forceinline__ bool past_end() const { return bitpos() > (uint64_t)end * 8u; }
};
typedef mk_bits_t<false> mk_bits;

/* the canonical walk, a bit at a time (codes longer than the look-up table's index, and every code an incomplete set leaves out) */
template <class B>
__device__ __forceinline__ int mk_decode_slow(B &b, const uint16_t *cnt, const uint16_t *sym) {
  int code = 0, first = 0, index = 0;
  for (uint32_t len = 1; len <= 15u; len++) {
    code |= (int)b.get(1);
    const int count = (int)mk_uni(cnt[len]);
    if (code - count < first) return (int)mk_uni(sym[index + (code - first)]);
    index += count;
    first += count;
    first <<= 1;
    code <<= 1;
  }
  return -1;
}
template <class B>
__device__ __forceinline__ int mk_decode(B &b, const uint16_t *tab, uint32_t bits, const uint16_t *cnt, const uint16_t *sym) {
  const uint32_t e = mk_uni(tab[(uint32_t)b.buf & ((1u << bits) - 1u)]);
  const uint32_t l = e & 15u;
  if (l) { b.buf >>= l; b.cnt -= l; return (int)(e >> 4); }
  return mk_decode_slow(b, cnt, sym);
}

/* code tables of n symbols with the lengths lens[]: 0 ok, 1 over-subscribed, 2 incomplete (allowed only for a single code of
 * length 1 or no code at all, as zlib does for literal/length and distance codes) */
__device__ int mk_build(const uint8_t *lens, uint32_t n, uint16_t *cnt, uint16_t *sym, uint16_t *tab, uint32_t bits, bool single_ok, uint32_t lane) {
  for (uint32_t i = lane; i < (1u << bits) / 2u; i += 64u) ((uint32_t *)tab)[i] = 0u;
  uint32_t c = 0;
  for (uint32_t s = 0; s < n; s++) c += (uint32_t)(lens[s] == lane); /* lane l: symbols of length l */
  if (lane == 0u || lane > 15u) c = 0;
  uint32_t offs = 0, first = 0, run = 0, code = 0, prevc = 0, maxlen = 0;
  int left = 1;
  bool over = false;
  for (uint32_t l = 1; l < 16u; l++) {
    const uint32_t cl = (uint32_t)__shfl((int)c, (int)l);
    left = (left << 1) - (int)cl;
    if (left < 0) over = true;
    code = (code + prevc) << 1;
    if (lane == l) { offs = run; first = code; }
    run += cl;
    prevc = cl;
    if (cl) maxlen = l;
  }
  if (lane < 16u) cnt[lane] = (uint16_t)c;
  if (over) return 1;
  if (left > 0 && !(single_ok && maxlen <= 1u)) return 2;
  if (c) { /* lanes 1..15 that have symbols: place them and fill the table */
    uint32_t k = 0;
    for (uint32_t s = 0; s < n && k < c; s++) {
      if (lens[s] != lane) continue;
      sym[offs + k] = (uint16_t)s;
      if (lane <= bits) {
        const uint32_t rev = __brev(first + k) >> (32u - lane);
        for (uint32_t e = rev; e < (1u << bits); e += 1u << lane) tab[e] = (uint16_t)(s << 4 | lane);
      }
      k++;
    }
  }
  mk_lds_fence();
  return 0;
}

/* The CRC register after the n >= 1 bytes at p, started from zero (ones: from all ones, n >= 4 then -- the start value is the
 * first four bytes complemented), by the whole wave: every lane runs the byte table over an equal slice (the bytes are thought
 * padded with zero bytes IN FRONT, which a zero register ignores), the 64 registers are folded with the 32x32 GF(2) matrix
 * "advance by one slice", squared at every level.  mat: 32 words of the wave's LDS.  The same value in every lane. */
__device__ __forceinline__ uint32_t mk_crc_wave(const uint8_t *p, uint32_t n, const uint32_t *crctab, uint32_t *mat, uint32_t lane, bool ones) {
  const uint32_t SL = (n + 63u) / 64u, pad = 64u * SL - n;
  uint32_t r = 0;
  for (uint32_t k = 0; k < SL; k++) {
    const uint32_t q = lane * SL + k;
    if (q >= pad) {
      const uint32_t idx = q - pad;
      uint32_t v = p[idx];
      if (ones && idx < 4u) v ^= 0xffu;
      r = crctab[(r ^ v) & 0xffu] ^ (r >> 8);
    }
  }
  { /* column j of "advance by SL zero bytes" */
    uint32_t m = 1u << (lane & 31u);
    for (uint32_t k = 0; k < SL; k++) m = crctab[m & 0xffu] ^ (m >> 8);
    mk_lds_fence();
    if (lane < 32u) mat[lane] = m;
    mk_lds_fence();
  }
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    uint32_t t = 0, col = 0;
    const uint32_t mine = mat[lane & 31u];
    for (uint32_t bit = 0; bit < 32u; bit++) {
      const uint32_t mb = mat[bit];
      if ((r >> bit) & 1u) t ^= mb;
      if ((mine >> bit) & 1u) col ^= mb;
    }
    const uint32_t u = (uint32_t)__shfl_up((int)t, d);
    if ((lane & (2u * d - 1u)) == 2u * d - 1u) r ^= u;
    mk_lds_fence();
    if (lane < 32u) mat[lane] = col; /* the matrix squared: twice the distance at the next level */
    mk_lds_fence();
  }
  return (uint32_t)__shfl((int)r, 63);
}

/* GZ: a plain gzip member of any size (mk_inflate_members, mk_sketch_batch_begin_gz).  No CRC on this wave -- mk_crc32_files_kernel
 * spreads it over the device --, a final block that ends before the payload is MK_INFL_TRAILING, and work[] (mk_gz.hip.h) takes
 * the bytes consumed and written beside the status.  Positions are 32-bit: a payload is below 2^31 bytes, a text at most
 * MK_BATCH_FILE_MAX, pos never passes isize + 258 before it is tested against it. */
template <bool GZ>
__global__ void __launch_bounds__(64 * MK_INFL_WAVES) mk_inflate_kernel(const uint8_t *__restrict__ comp, const mk_infl_blk *__restrict__ blks,
                                                                         uint32_t nblocks, uint8_t *text, uint32_t *status) {
  __shared__ mk_infl_lds lds_all[MK_INFL_WAVES];
  __shared__ uint32_t crctab[256];
  {
    uint32_t c = threadIdx.x;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    crctab[threadIdx.x] = c;
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t blk = blockIdx.x * MK_INFL_WAVES + wave;
  if (blk >= nblocks) return;
  mk_infl_lds &L = lds_all[wave];
  const mk_infl_blk B = blks[blk];
  const uint32_t isize = mk_uni(B.isize);
  uint8_t *out = text + mk_uni(B.out_off);
  const uint32_t shift = mk_uni(B.pay_off) & 15u;
  mk_bits b;
  b.base = comp + (mk_uni(B.pay_off) - shift);
  b.win = L.win;
  b.end = shift + mk_uni(B.pay_len);
  b.lane = lane;
  b.seek(shift);

  uint32_t st = MK_INFL_OK, pos = 0, nlit = 0, synced = 0, lit = 0;
  /* pending literals -> one store; false: they do not fit */
  auto flush = [&]() -> bool {
    if (nlit) {
      if (pos + nlit > isize) { nlit = 0; return false; }
      if (lane < nlit) out[pos + lane] = (uint8_t)lit;
      pos += nlit;
      nlit = 0;
    }
    return true;
  };
  uint32_t last = 0;
  do {
    b.refill();
    if (b.past_end()) { st = MK_INFL_INPUT; break; }
    last = b.get(1);
    const uint32_t type = b.get(2);
    if (type == 0u) { /* stored: LEN bytes behind LEN, NLEN at the next byte boundary */
      b.get(b.cnt & 7u);
      b.refill();
      const uint32_t len = b.get(16), nlen = b.get(16);
      if ((len ^ nlen) != 0xffffu) { st = MK_INFL_BAD_BLOCK; break; }
      const uint32_t a0 = (uint32_t)(b.bitpos() >> 3);
      if (b.past_end() || a0 + len > b.end) { st = MK_INFL_INPUT; break; }
      if (!flush() || pos + len > isize) { st = MK_INFL_OUTPUT_LEN; break; }
      for (uint32_t i = lane; i < len; i += 64u) out[pos + i] = b.base[a0 + i];
      pos += len;
      b.seek(a0 + len);
      continue;
    }
    if (type == 3u) { st = MK_INFL_BAD_BLOCK; break; }
    uint32_t nl = 288u, nd = 32u;
    if (type == 1u) {
      for (uint32_t i = lane; i < 320u; i += 64u) L.lens[i] = (uint8_t)(i < 144u ? 8u : i < 256u ? 9u : i < 280u ? 7u : i < 288u ? 8u : 5u);
      mk_lds_fence();
    } else {
      nl = b.get(5) + 257u;
      nd = b.get(5) + 1u;
      const uint32_t nc = b.get(4) + 4u;
      if (nl > 286u || nd > 30u) { st = MK_INFL_BAD_LENGTHS; break; }
      if (lane < 19u) L.lens[320u + lane] = 0;
      mk_lds_fence();
      for (uint32_t i = 0; i < nc; i++) {
        b.refill();
        const uint32_t v = b.get(3);
        if (lane == 0u) L.lens[320u + mk_clorder[i]] = (uint8_t)v;
      }
      mk_lds_fence();
      /* the code length code borrows the distance code's arrays; 7 bits index its whole table */
      if (mk_build(L.lens + 320, 19u, L.dist_cnt, L.dist_sym, L.dist_tab, 7u, false, lane)) { st = MK_INFL_BAD_CODE; break; }
      uint32_t idx = 0, prev = 0;
      while (idx < nl + nd) {
        b.refill();
        if (b.past_end()) { st = MK_INFL_INPUT; break; }
        const int s = mk_decode(b, L.dist_tab, 7u, L.dist_cnt, L.dist_sym);
        if (s < 0) { st = MK_INFL_BAD_CODE; break; }
        if (s < 16) {
          if (lane == 0u) L.lens[idx] = (uint8_t)s;
          prev = (uint32_t)s;
          idx++;
          continue;
        }
        uint32_t rep, val = 0;
        if (s == 16) {
          if (idx == 0u) { st = MK_INFL_BAD_LENGTHS; break; }
          val = prev;
          rep = 3u + b.get(2);
        } else if (s == 17) rep = 3u + b.get(3);
        else rep = 11u + b.get(7);
        if (idx + rep > nl + nd) { st = MK_INFL_BAD_LENGTHS; break; }
        for (uint32_t i = lane; i < rep; i += 64u) L.lens[idx + i] = (uint8_t)val;
        prev = val;
        idx += rep;
      }
      if (st) break;
      mk_lds_fence();
      if (L.lens[256] == 0) { st = MK_INFL_BAD_LENGTHS; break; }
    }
    if (mk_build(L.lens, nl, L.lit_cnt, L.lit_sym, L.lit_tab, MK_INFL_LBITS, true, lane) ||
        mk_build(L.lens + nl, nd, L.dist_cnt, L.dist_sym, L.dist_tab, MK_INFL_DBITS, true, lane)) { st = MK_INFL_BAD_CODE; break; }
    /* the tokens of this block: each takes at least one bit of input */
    for (;;) {
      b.refill();
      if (b.past_end()) { st = MK_INFL_INPUT; break; }
      int s = mk_decode(b, L.lit_tab, MK_INFL_LBITS, L.lit_cnt, L.lit_sym);
      if (s < 0) { st = MK_INFL_BAD_CODE; break; }
      if (s < 256) {
        if (lane == nlit) lit = (uint32_t)s;
        if (++nlit == 64u && !flush()) { st = MK_INFL_OUTPUT_LEN; break; }
        continue;
      }
      if (s == 256) break;
      s -= 257;
      if (s >= 29) { st = MK_INFL_BAD_CODE; break; }
      const uint32_t len = (uint32_t)mk_lbase[s] + b.get(mk_lext[s]);
      b.refill();
      const int d = mk_decode(b, L.dist_tab, MK_INFL_DBITS, L.dist_cnt, L.dist_sym);
      if (d < 0) { st = MK_INFL_BAD_CODE; break; }
      if (d >= 30) { st = MK_INFL_BAD_DISTANCE; break; }
      const uint32_t dist = (uint32_t)mk_dbase[d] + b.get(mk_dext[d]);
      if (!flush()) { st = MK_INFL_OUTPUT_LEN; break; }
      if (dist > pos) { st = MK_INFL_BAD_DISTANCE; break; }
      if (pos + len > isize) { st = MK_INFL_OUTPUT_LEN; break; }
      const uint32_t from = pos - dist;
      if (from + (len < dist ? len : dist) > synced) { mk_store_fence(); synced = pos; } /* the source was written since the last wait */
      if (dist >= len) { for (uint32_t i = lane; i < len; i += 64u) out[pos + i] = out[from + i]; }
      else { for (uint32_t i = lane; i < len; i += 64u) out[pos + i] = out[from + i % dist]; }
      pos += len;
    }
    if (st) break;
  } while (!last);
  if (!st && !flush()) st = MK_INFL_OUTPUT_LEN;
  if (!st && b.past_end()) st = MK_INFL_INPUT;
  if (GZ) {
    uint64_t used = (b.bitpos() + 7u) >> 3;
    if (used > b.end) used = b.end;
    const uint32_t consumed = (uint32_t)used - shift;
    if (!st && consumed < mk_uni(B.pay_len)) st = MK_INFL_TRAILING;
    if (!st && pos != isize) st = MK_INFL_OUTPUT_LEN;
    if (lane == 0u) { status[blk] = st; status[nblocks + blk] = consumed; status[2u * nblocks + blk] = pos; }
    return;
  }
  if (!st && pos != isize) st = MK_INFL_OUTPUT_LEN;

  if (!st) { /* CRC32 of out[0, isize) */
    mk_store_fence();
    uint32_t crc;
    if (isize < 256u) {
      uint32_t c = 0xffffffffu;
      for (uint32_t i = 0; i < isize; i++) c = crctab[(c ^ out[i]) & 0xffu] ^ (c >> 8);
      crc = ~c;
    } else {
      crc = ~mk_crc_wave(out, isize, crctab, L.mat, lane, true);
    }
    if (crc != mk_uni(B.crc)) st = MK_INFL_CRC;
  }
  if (lane == 0u) status[blk] = st;
}

/* ---- CRC32 of many texts, many waves per text -------------------------------------------------------------------------------------
 * Slice s of the launch is slice s - slice0s[f] of member f: MK_CRC_SLICE bytes of its text (the last one what is left), one wave.
 * What it leaves is the register started from ZERO: registers of neighbouring slices combine linearly. */
__global__ void __launch_bounds__(256) mk_crc32_files_kernel(const uint8_t *__restrict__ text, const mk_infl_blk *__restrict__ blks, const uint32_t *__restrict__ slice0s,
                                                             uint32_t nfiles, uint32_t nslices, uint32_t *slice_crc) {
  __shared__ uint32_t crctab[256];
  __shared__ uint32_t mat[4][32];
  {
    uint32_t c = threadIdx.x;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    crctab[threadIdx.x] = c;
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t s = blockIdx.x * 4u + wave;
  if (s >= nslices) return;
  uint32_t lo = 0, hi = nfiles; /* the last member whose first slice is <= s (members without text share their successor's) */
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (slice0s[mid] <= s) lo = mid; else hi = mid;
  }
  const uint32_t f = lo;
  const uint32_t isize = mk_uni(blks[f].isize), at = (s - mk_uni(slice0s[f])) * MK_CRC_SLICE;
  if (at >= isize) return; /* (cannot happen: the host counted the slices from the same sizes) */
  const uint32_t n = isize - at < MK_CRC_SLICE ? isize - at : MK_CRC_SLICE;
  const uint32_t r = mk_crc_wave(text + mk_uni(blks[f].out_off) + at, n, crctab, mat[wave], lane, false);
  if (lane == 0u) slice_crc[s] = r;
}

/* a * b mod the CRC polynomial, bit-reflected (x^0 is bit 31); x^(8n), which advances a register over n zero bytes */
__device__ __forceinline__ uint32_t mk_crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
  }
  return p;
}
__device__ __forceinline__ uint32_t mk_crc_xpow8(uint32_t n) {
  uint32_t p = 1u << 31, sq = 0x00800000u;
  for (; n; n >>= 1) {
    if (n & 1u) p = mk_crc_mul(sq, p);
    sq = mk_crc_mul(sq, sq);
  }
  return p;
}
/* one THREAD per member: its slices' registers in order, each advanced over what follows it; the all-ones start value advanced over
 * the whole text and the final complement; the comparison with the trailer goes into a status that was MK_INFL_OK */
__global__ void __launch_bounds__(64) mk_crc32_combine_kernel(const mk_infl_blk *__restrict__ blks, const uint32_t *__restrict__ slice0s, uint32_t nfiles,
                                                              const uint32_t *__restrict__ slice_crc, uint32_t *status, uint32_t *crc_out) {
  const uint32_t f = blockIdx.x * 64u + threadIdx.x;
  if (f >= nfiles) return;
  const uint32_t isize = blks[f].isize, s0 = slice0s[f], ns = slice0s[f + 1u] - s0;
  const uint32_t xfull = mk_crc_xpow8(MK_CRC_SLICE);
  uint32_t tot = 0;
  for (uint32_t j = 0; j < ns; j++) {
    const uint32_t len = j + 1u < ns ? MK_CRC_SLICE : isize - j * MK_CRC_SLICE;
    tot = mk_crc_mul(len == MK_CRC_SLICE ? xfull : mk_crc_xpow8(len), tot) ^ slice_crc[s0 + j];
  }
  const uint32_t crc = ~(tot ^ mk_crc_mul(mk_crc_xpow8(isize), 0xffffffffu));
  crc_out[f] = crc;
  if (status[f] == MK_INFL_OK && crc != blks[f].crc) status[f] = MK_INFL_CRC;
}

double mk_now_s() {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

} /* namespace */

/* *p holds `need` elements afterwards (device memory, or pinned host memory): grown with room to spare, what it held is lost */
template <class T>
static hipError_t mk_grow(T **p, uint64_t *cap, uint64_t need, bool pinned) {
  if (need == 0) need = 1;
  if (*p && need <= *cap) return hipSuccess;
  if (*p) { if (pinned) (void)hipHostFree(*p); else (void)hipFree(*p); }
  *p = nullptr; *cap = 0;
  const uint64_t c = need + need / 8 + 256;
  const hipError_t r = pinned ? mk_pin_alloc(p, c * sizeof(T), hipHostMallocDefault) : mk_dev_alloc(p, c * sizeof(T));
  if (r == hipSuccess) *cap = c;
  return r;
}

#include "mk_fq_frame.hip.h"

struct mk_inflate {
  int device = 0;
  hipStream_t stream = nullptr;
  /* the test entry points' buffers (mk_sketch_push_bgzf keeps its own) */
  uint8_t *h_stage = nullptr, *d_comp = nullptr, *d_text = nullptr;
  uint64_t stage_cap = 0, comp_cap = 0, text_cap = 0;
  uint32_t *d_status = nullptr, *h_status = nullptr;
  uint64_t status_cap = 0, h_status_cap = 0;
  mk_fq_framer fq; /* mk_fastq_frame_device, mk_fastq_frame_q_device */
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  double inflate_ms = 0.0, frame_ms = 0.0;
  uint64_t stream_members = 0; /* of the last mk_inflate_stream */
  uint64_t stream_repairs = 0; /* ... and the starts its repair dropped (MK_GUNZIP_REPAIR) */
  char err[256] = {0};
};

static thread_local char mk_inflate_create_err[256];

static int mk_infl_fail(mk_inflate *h, int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(h ? h->err : mk_inflate_create_err, 256, fmt, ap);
  va_end(ap);
  return code;
}

#define MK_INFL_HIP(h, call)                                                                          \
  do {                                                                                                \
    hipError_t _r = (call);                                                                           \
    if (_r != hipSuccess) return mk_infl_fail(h, MK_ERR_HIP, "%s: %s", #call, hipGetErrorString(_r)); \
  } while (0)

extern "C" int mk_inflate_create(int device, mk_inflate **out) {
  if (!out) return MK_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return mk_infl_fail(nullptr, MK_ERR_NO_DEVICE, "no HIP device: mk_inflate has no CPU path");
  if (device < 0 || device >= ndev) return mk_infl_fail(nullptr, MK_ERR_NO_DEVICE, "device %d out of range (0..%d)", device, ndev - 1);
  mk_inflate *h = new (std::nothrow) mk_inflate();
  if (!h) return MK_ERR_NOMEM;
  h->device = device;
  if (hipSetDevice(device) != hipSuccess) {
    delete h;
    return mk_infl_fail(nullptr, MK_ERR_NO_DEVICE, "hipSetDevice(%d) failed", device);
  }
  hipError_t r = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (r == hipSuccess) r = h->fq.setup(false, 0);
  for (int i = 0; i < 4 && r == hipSuccess; i++) r = hipEventCreate(&h->ev[i]);
  if (r != hipSuccess) {
    mk_infl_fail(nullptr, MK_ERR_NOMEM, "inflate allocation: %s", hipGetErrorString(r));
    mk_inflate_destroy(h);
    return MK_ERR_NOMEM;
  }
  *out = h;
  return MK_OK;
}

extern "C" int mk_inflate_destroy(mk_inflate *h) {
  if (!h) return MK_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  void *dev[] = {h->d_comp, h->d_text, h->d_status};
  for (void *p : dev) (void)hipFree(p);
  void *pin[] = {h->h_stage, h->h_status};
  for (void *p : pin) if (p) (void)hipHostFree(p);
  for (hipEvent_t e : h->ev) if (e) (void)hipEventDestroy(e);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return MK_OK;
}

extern "C" const char *mk_inflate_last_error(const mk_inflate *h) { return h ? h->err : mk_inflate_create_err; }

extern "C" int mk_inflate_last_kernel_ms(mk_inflate *h, double *inflate_ms, double *frame_ms) {
  if (!h) return MK_ERR_ARG;
  if (inflate_ms) *inflate_ms = h->inflate_ms;
  if (frame_ms) *frame_ms = h->frame_ms;
  return MK_OK;
}

/* ---- launches, on any stream ------------------------------------------------------------------------------------------------ */
static hipError_t mk_launch_inflate(hipStream_t s, const uint8_t *d_comp, const mk_infl_blk *d_blks, uint32_t nblocks, uint8_t *d_text, uint32_t *d_status) {
  if (!nblocks) return hipSuccess;
  hipLaunchKernelGGL(mk_inflate_kernel<false>, dim3((nblocks + MK_INFL_WAVES - 1) / MK_INFL_WAVES), dim3(64 * MK_INFL_WAVES), 0, s, d_comp, d_blks, nblocks, d_text, d_status);
  return hipGetLastError();
}
hipError_t mk_gz_launch(hipStream_t s, const uint8_t *d_comp, const void *d_tab, uint32_t n, uint32_t nslices, uint8_t *d_text, uint32_t *d_work) {
  if (!n) return hipSuccess;
  const mk_infl_blk *blks = (const mk_infl_blk *)d_tab;
  const uint32_t *slice0s = (const uint32_t *)((const uint8_t *)d_tab + mk_gz_slice0_at(n));
  hipLaunchKernelGGL(mk_inflate_kernel<true>, dim3((n + MK_INFL_WAVES - 1) / MK_INFL_WAVES), dim3(64 * MK_INFL_WAVES), 0, s, d_comp, blks, n, d_text, d_work);
  if (nslices) hipLaunchKernelGGL(mk_crc32_files_kernel, dim3((nslices + 3u) / 4u), dim3(256), 0, s, (const uint8_t *)d_text, blks, slice0s, n, nslices, d_work + 4u * (size_t)n);
  hipLaunchKernelGGL(mk_crc32_combine_kernel, dim3((n + 63u) / 64u), dim3(64), 0, s, blks, slice0s, n, (const uint32_t *)(d_work + 4u * (size_t)n), d_work, d_work + 3u * (size_t)n);
  return hipGetLastError();
}
/* ---- the two entry points with a copy-back (tests, tools) ---------------------------------------------------------------------- */
extern "C" int mk_inflate_blocks(mk_inflate *h, const uint8_t *comp, size_t comp_bytes, const mk_bgzf_block *blocks, uint64_t nblocks,
                                 uint8_t *out_host, size_t out_cap, uint32_t *status) {
  if (!h || (!comp && comp_bytes) || (!blocks && nblocks) || !status) return MK_ERR_ARG;
  if (nblocks == 0) return MK_OK;
  if (nblocks > (1u << 24) || comp_bytes >= (1ull << 31)) return mk_infl_fail(h, MK_ERR_ARG, "mk_inflate_blocks: at most 2^24 members and 2 GiB a call");
  uint64_t text_end = 0;
  for (uint64_t i = 0; i < nblocks; i++) {
    const mk_bgzf_block &b = blocks[i];
    if (b.in_off + b.pay_off + (uint64_t)b.pay_len > comp_bytes || b.isize > 65536u || b.out_off + b.isize >= (1ull << 31))
      return mk_infl_fail(h, MK_ERR_ARG, "mk_inflate_blocks: member %llu lies outside the buffers", (unsigned long long)i);
    if (b.out_off + b.isize > text_end) text_end = b.out_off + b.isize;
  }
  if (out_host && out_cap < text_end) return mk_infl_fail(h, MK_ERR_ARG, "mk_inflate_blocks: out_cap too small");
  MK_INFL_HIP(h, hipSetDevice(h->device));
  const uint64_t tab_at = (comp_bytes + 15u) & ~(uint64_t)15u, stage_bytes = tab_at + nblocks * sizeof(mk_infl_blk);
  MK_INFL_HIP(h, mk_grow(&h->h_stage, &h->stage_cap, stage_bytes, true));
  MK_INFL_HIP(h, mk_grow(&h->d_comp, &h->comp_cap, stage_bytes + 64, false));
  MK_INFL_HIP(h, mk_grow(&h->d_text, &h->text_cap, mk_fq_buf_bytes(text_end), false));
  MK_INFL_HIP(h, mk_grow(&h->d_status, &h->status_cap, nblocks, false));
  MK_INFL_HIP(h, mk_grow(&h->h_status, &h->h_status_cap, nblocks, true));
  memcpy(h->h_stage, comp, comp_bytes);
  mk_infl_blk *tab = (mk_infl_blk *)(h->h_stage + tab_at);
  for (uint64_t i = 0; i < nblocks; i++) {
    const mk_bgzf_block &b = blocks[i];
    tab[i] = mk_infl_blk{(uint32_t)(b.in_off + b.pay_off), b.pay_len, (uint32_t)b.out_off, b.isize, b.crc32};
  }
  MK_INFL_HIP(h, hipMemcpyAsync(h->d_comp, h->h_stage, stage_bytes, hipMemcpyHostToDevice, h->stream));
  MK_INFL_HIP(h, hipEventRecord(h->ev[0], h->stream));
  MK_INFL_HIP(h, mk_launch_inflate(h->stream, h->d_comp, (const mk_infl_blk *)(h->d_comp + tab_at), (uint32_t)nblocks, h->d_text, h->d_status));
  MK_INFL_HIP(h, hipEventRecord(h->ev[1], h->stream));
  MK_INFL_HIP(h, hipMemcpyAsync(h->h_status, h->d_status, nblocks * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  MK_INFL_HIP(h, hipStreamSynchronize(h->stream));
  memcpy(status, h->h_status, nblocks * sizeof(uint32_t));
  if (out_host && text_end) MK_INFL_HIP(h, hipMemcpy(out_host, h->d_text, text_end, hipMemcpyDeviceToHost));
  float ms = 0.f;
  MK_INFL_HIP(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  h->inflate_ms = ms;
  return MK_OK;
}

extern "C" int mk_inflate_members(mk_inflate *h, const uint8_t *comp, size_t comp_bytes, const mk_gz_member *members, uint32_t nmembers,
                                  uint8_t *out_host, size_t out_cap, mk_gz_member_result *res) {
  if (!h || (!comp && comp_bytes) || (!members && nmembers) || !res) return MK_ERR_ARG;
  if (nmembers == 0) return MK_OK;
  if (nmembers > (1u << 20) || comp_bytes >= (1ull << 31)) return mk_infl_fail(h, MK_ERR_ARG, "mk_inflate_members: at most 2^20 members and 2 GiB a call");
  uint64_t text_end = 0, nslices = 0;
  for (uint32_t i = 0; i < nmembers; i++) {
    const mk_gz_member &m = members[i];
    if (m.pay_off + (uint64_t)m.pay_len > comp_bytes || m.isize > MK_BATCH_FILE_MAX || m.out_off + m.isize > (1ull << 30))
      return mk_infl_fail(h, MK_ERR_ARG, "mk_inflate_members: member %u lies outside the buffers", i);
    if (m.out_off + m.isize > text_end) text_end = m.out_off + m.isize;
    nslices += mk_gz_slices(m.isize);
  }
  if (out_host && out_cap < text_end) return mk_infl_fail(h, MK_ERR_ARG, "mk_inflate_members: out_cap too small");
  MK_INFL_HIP(h, hipSetDevice(h->device));
  const uint64_t tab_at = (comp_bytes + 15u) & ~(uint64_t)15u, stage_bytes = tab_at + mk_gz_table_bytes(nmembers);
  const uint64_t words = mk_gz_work_words(nmembers, (uint32_t)nslices);
  MK_INFL_HIP(h, mk_grow(&h->h_stage, &h->stage_cap, stage_bytes, true));
  MK_INFL_HIP(h, mk_grow(&h->d_comp, &h->comp_cap, stage_bytes + 64, false));
  MK_INFL_HIP(h, mk_grow(&h->d_text, &h->text_cap, mk_fq_buf_bytes(text_end), false));
  MK_INFL_HIP(h, mk_grow(&h->d_status, &h->status_cap, words, false));
  MK_INFL_HIP(h, mk_grow(&h->h_status, &h->h_status_cap, 4u * (uint64_t)nmembers, true));
  memcpy(h->h_stage, comp, comp_bytes);
  memset(h->h_stage + comp_bytes, 0, tab_at - comp_bytes);
  mk_infl_blk *tab = (mk_infl_blk *)(h->h_stage + tab_at);
  uint32_t *slice0s = (uint32_t *)(h->h_stage + tab_at + mk_gz_slice0_at(nmembers));
  uint32_t s0 = 0;
  for (uint32_t i = 0; i < nmembers; i++) {
    const mk_gz_member &m = members[i];
    tab[i] = mk_infl_blk{(uint32_t)m.pay_off, m.pay_len, (uint32_t)m.out_off, m.isize, m.crc32};
    slice0s[i] = s0;
    s0 += mk_gz_slices(m.isize);
  }
  slice0s[nmembers] = s0;
  MK_INFL_HIP(h, hipMemcpyAsync(h->d_comp, h->h_stage, stage_bytes, hipMemcpyHostToDevice, h->stream));
  MK_INFL_HIP(h, hipEventRecord(h->ev[0], h->stream));
  MK_INFL_HIP(h, mk_gz_launch(h->stream, h->d_comp, h->d_comp + tab_at, nmembers, s0, h->d_text, h->d_status));
  MK_INFL_HIP(h, hipEventRecord(h->ev[1], h->stream));
  MK_INFL_HIP(h, hipMemcpyAsync(h->h_status, h->d_status, 4u * (size_t)nmembers * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  MK_INFL_HIP(h, hipStreamSynchronize(h->stream));
  for (uint32_t i = 0; i < nmembers; i++)
    res[i] = mk_gz_member_result{h->h_status[i], h->h_status[nmembers + i], h->h_status[2u * (size_t)nmembers + i], h->h_status[3u * (size_t)nmembers + i]};
  if (out_host && text_end) MK_INFL_HIP(h, hipMemcpy(out_host, h->d_text, text_end, hipMemcpyDeviceToHost));
  float ms = 0.f;
  MK_INFL_HIP(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  h->inflate_ms = ms;
  return MK_OK;
}

#define MK_FRAME_PORTION ((uint64_t)1 << 20) /* row bytes the test entries take back at a time: the routes' portion loop at small sizes */

/* both entries: occ == false is mk_fastq_frame's rule, occ == true mk_fastq_frame_q's (qmin, records_before) */
static int mk_frame_device(mk_inflate *h, const char *who, bool occ, const uint8_t *text, size_t n, int final, int32_t qmin, uint64_t records_before,
                           uint8_t *rows_host, size_t rows_cap, uint32_t *stride, uint64_t *nrows, size_t *consumed, uint32_t *longest) {
  if (n >= (1ull << 30)) return mk_infl_fail(h, MK_ERR_ARG, "%s: at most 2^30 bytes a call", who);
  MK_INFL_HIP(h, hipSetDevice(h->device));
  mk_fq_framer &F = h->fq;
  const uint32_t e1 = (uint32_t)n;
  MK_INFL_HIP(h, F.setup(occ, qmin));
  MK_INFL_HIP(h, mk_grow(&h->d_text, &h->text_cap, mk_fq_buf_bytes(e1), false));
  MK_INFL_HIP(h, F.reserve(h->stream, e1, MK_FRAME_PORTION));
  if (n) MK_INFL_HIP(h, hipMemcpyAsync(h->d_text, text, n, hipMemcpyHostToDevice, h->stream));
  MK_INFL_HIP(h, hipEventRecord(h->ev[2], h->stream));
  MK_INFL_HIP(h, F.count(h->stream, h->d_text, 0, e1, final != 0, nullptr, 0));
  mk_fq_chunk c;
  MK_INFL_HIP(h, F.result(records_before, &c));
  if (longest) *longest = c.r.maxline;
  *nrows = 0; *consumed = 0; *stride = c.stride;
  if (c.long_line) return mk_infl_fail(h, MK_ERR_FORMAT, "a FASTQ line of 4095 characters or more");
  uint64_t at = 0; /* row bytes copied back so far */
  auto push = [&](const uint8_t *d_rows, uint32_t sd, uint32_t k) -> int {
    if (!rows_host) return MK_OK;
    const uint32_t all = c.first ? k : c.r.nrec; /* (the first record's row is the only one) */
    if ((uint64_t)all * sd > rows_cap) return mk_infl_fail(h, MK_ERR_ARG, "%s: %u rows of %u bytes do not fit rows_cap", who, all, sd);
    MK_INFL_HIP(h, hipMemcpyAsync(rows_host + at, d_rows, (uint64_t)k * sd, hipMemcpyDeviceToHost, h->stream));
    at += (uint64_t)k * sd;
    return MK_OK;
  };
  mk_fq_handed out;
  MK_INFL_HIP(h, F.rows(h->stream, c, push, &out));
  *stride = out.stride;
  if (out.push_rc) { (void)hipStreamSynchronize(h->stream); return out.push_rc; }
  MK_INFL_HIP(h, hipEventRecord(h->ev[3], h->stream));
  MK_INFL_HIP(h, hipStreamSynchronize(h->stream));
  float ms = 0.f;
  MK_INFL_HIP(h, hipEventElapsedTime(&ms, h->ev[2], h->ev[3]));
  h->frame_ms = ms;
  *nrows = out.rows;
  *consumed = c.r.consumed;
  return MK_OK;
}

extern "C" int mk_fastq_frame_device(mk_inflate *h, const uint8_t *text, size_t n, int final, uint8_t *rows_host, size_t rows_cap,
                                     uint32_t *stride, uint64_t *nrows, size_t *consumed, uint32_t *longest) {
  if (!h || (!text && n) || !stride || !nrows || !consumed) return MK_ERR_ARG;
  return mk_frame_device(h, "mk_fastq_frame_device", false, text, n, final, 0, 0, rows_host, rows_cap, stride, nrows, consumed, longest);
}

extern "C" int mk_fastq_frame_q_device(mk_inflate *h, const uint8_t *text, size_t n, int final, int32_t qmin, uint64_t records_before,
                                       uint8_t *rows_host, size_t rows_cap, uint32_t *stride, uint64_t *nrows, uint64_t *nrecords,
                                       size_t *consumed, uint32_t *longest) {
  if (!h || (!text && n) || !stride || !nrows || !nrecords || !consumed) return MK_ERR_ARG;
  *nrecords = 0;
  const int rc = mk_frame_device(h, "mk_fastq_frame_q_device", true, text, n, final, qmin, records_before, rows_host, rows_cap, stride, nrows, consumed, longest);
  if (rc == MK_OK) *nrecords = *nrows;
  return rc;
}

/* ---- the route bound to an engine -------------------------------------------------------------------------------------------- */
namespace {
struct mk_bgzf_run { /* everything mk_sketch_push_bgzf allocates beside its framer, released on every way out */
  mk_bgzf_block *blocks = nullptr;
  hipStream_t copy = nullptr;
  uint8_t *h_stage[2] = {nullptr, nullptr}, *d_comp[2] = {nullptr, nullptr}, *d_text[2] = {nullptr, nullptr};
  uint32_t *d_status[2] = {nullptr, nullptr};
  uint32_t *d_bad = nullptr, *h_bad = nullptr; /* the long sink: mk_bgzf_bad_kernel's two words and their pinned mirror */
  hipEvent_t ev_bad = nullptr;
  hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_i[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  ~mk_bgzf_run() {
    mk_bgzf_free(blocks);
    for (int s = 0; s < 2; s++) {
      if (h_stage[s]) (void)hipHostFree(h_stage[s]);
      (void)hipFree(d_comp[s]); (void)hipFree(d_text[s]); (void)hipFree(d_status[s]);
      if (ev_up[s]) (void)hipEventDestroy(ev_up[s]);
      for (int k = 0; k < 2; k++) if (ev_i[s][k]) (void)hipEventDestroy(ev_i[s][k]);
    }
    (void)hipFree(d_bad);
    if (h_bad) (void)hipHostFree(h_bad);
    if (ev_bad) (void)hipEventDestroy(ev_bad);
    if (copy) (void)hipStreamDestroy(copy);
  }
};
struct mk_bgzf_chunk { uint64_t b0, b1, in0, in1, text; };

/* the long sink has no framer whose scan kernel reduces the members' statuses: one workgroup does that alone.
 * out[0] := the first member of the chunk with a status (0xffffffff: none), out[1] := that status */
__global__ void __launch_bounds__(1024) mk_bgzf_bad_kernel(const uint32_t *status, uint32_t nblocks, uint32_t *out) {
  __shared__ uint32_t s_bad;
  if (threadIdx.x == 0u) s_bad = 0xffffffffu;
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < nblocks; i += 1024u) if (status[i]) atomicMin(&s_bad, i);
  __syncthreads();
  if (threadIdx.x == 0u) { out[0] = s_bad; out[1] = s_bad != 0xffffffffu ? status[s_bad] : 0u; }
}
}

static thread_local char mk_bgzf_err[256];
#define MK_BGZF_HIP(call)                                                                                             \
  do {                                                                                                                \
    hipError_t _r = (call);                                                                                           \
    if (_r != hipSuccess) { snprintf(mk_bgzf_err, sizeof mk_bgzf_err, "%s: %s", #call, hipGetErrorString(_r)); (void)hipStreamSynchronize(S); if (R.copy) (void)hipStreamSynchronize(R.copy); return MK_ERR_HIP; } \
  } while (0)

/* both readers' route: occ == false is mk_fastq_frame's rule (-A), occ == true mk_fastq_frame_q's (quality mask qmin).  lng: the long
 * sink -- scan, chunks, upload and inflate are the same; a chunk's text goes to mk_sketch_push_fastq_long_device
 * instead of the framer (occ: to mk_sketch_push_fastq_long_q_device with qmin, 4.21), `final` with the file's last chunk when final_in
 * says the sketch ends with this file. */
static int mk_push_bgzf(mk_engine *e, int fd, size_t size, const mk_bgzf_opts *o, bool occ, int32_t qmin, uint64_t first_ordinal, mk_bgzf_stats *st,
                        bool lng = false, int final_in = 1) {
  if (!e || fd < 0) return MK_ERR_ARG;
  mk_bgzf_stats stats;
  memset(&stats, 0, sizeof stats);
  stats.bad_block = -1;
  if (st) *st = stats;
  const double t_begin = mk_now_s();
  mk_bgzf_run R;
  uint64_t nblocks = 0, total = 0;
  int is_bgzf = 0;
  int rc = mk_bgzf_scan(fd, nullptr, size, &R.blocks, &nblocks, &total, &is_bgzf);
  if (rc) return rc;
  if (!is_bgzf) return MK_ERR_ARG;
  stats.t_scan_s = mk_now_s() - t_begin;
  void *sp = nullptr;
  int device = 0;
  rc = mk_engine_get_stream(e, &sp, &device);
  if (rc) return rc;
  hipStream_t S = (hipStream_t)sp;
  /* chunks: runs of members whose text stays within chunk_bytes (at least one member each) */
  uint64_t chunk_bytes = o && o->chunk_bytes ? o->chunk_bytes : (uint64_t)128 << 20;
  if (chunk_bytes < 65536u) chunk_bytes = 65536u;
  if (chunk_bytes > ((uint64_t)1 << 30)) chunk_bytes = (uint64_t)1 << 30;
  std::vector<mk_bgzf_chunk> chunks;
  uint64_t max_in = 0, max_text = 0, max_blocks = 0;
  for (uint64_t b = 0; b < nblocks;) {
    mk_bgzf_chunk c{b, b, R.blocks[b].in_off, 0, 0};
    while (c.b1 < nblocks && (c.b1 == c.b0 || c.text + R.blocks[c.b1].isize <= chunk_bytes)) c.text += R.blocks[c.b1++].isize;
    c.in1 = R.blocks[c.b1 - 1].in_off + R.blocks[c.b1 - 1].in_len;
    if (c.in1 - c.in0 >= ((uint64_t)1 << 31)) { snprintf(mk_bgzf_err, sizeof mk_bgzf_err, "a chunk of more than 2 GiB of compressed bytes"); return MK_ERR_ARG; }
    max_in = c.in1 - c.in0 > max_in ? c.in1 - c.in0 : max_in;
    max_text = c.text > max_text ? c.text : max_text;
    max_blocks = c.b1 - c.b0 > max_blocks ? c.b1 - c.b0 : max_blocks;
    chunks.push_back(c);
    b = c.b1;
  }
  const uint64_t stage_bytes = ((max_in + 15u) & ~(uint64_t)15u) + max_blocks * sizeof(mk_infl_blk);
  const uint64_t text_bytes = mk_fq_buf_bytes(MK_FQ_CARRY + max_text);
  const uint64_t rows_bytes = (max_text + MK_FQ_CARRY > ((uint64_t)8 << 20) ? max_text + MK_FQ_CARRY : (uint64_t)8 << 20) + 4096u;
  MK_BGZF_HIP(hipSetDevice(device));
  MK_BGZF_HIP(hipStreamCreateWithFlags(&R.copy, hipStreamNonBlocking));
  for (int s = 0; s < 2; s++) {
    if (s == 1 && chunks.size() < 2) break;
    MK_BGZF_HIP(mk_pin_alloc(&R.h_stage[s], stage_bytes, hipHostMallocDefault));
    MK_BGZF_HIP(mk_dev_alloc(&R.d_comp[s], stage_bytes + 64));
    MK_BGZF_HIP(mk_dev_alloc(&R.d_text[s], text_bytes));
    MK_BGZF_HIP(mk_dev_alloc(&R.d_status[s], max_blocks * sizeof(uint32_t)));
    MK_BGZF_HIP(hipEventCreateWithFlags(&R.ev_up[s], hipEventDisableTiming));
    for (int k = 0; k < 2; k++) MK_BGZF_HIP(hipEventCreate(&R.ev_i[s][k]));
  }
  mk_fq_framer F;
  double frame0 = 0;
  if (lng) {
    MK_BGZF_HIP(mk_dev_alloc(&R.d_bad, 2 * sizeof(uint32_t)));
    MK_BGZF_HIP(mk_pin_alloc(&R.h_bad, 2 * sizeof(uint32_t), hipHostMallocDefault));
    MK_BGZF_HIP(hipEventCreateWithFlags(&R.ev_bad, hipEventDisableTiming));
    if ((rc = mk_sketch_fastq_long_frame_ms(e, &frame0))) { snprintf(mk_bgzf_err, sizeof mk_bgzf_err, "%s", mk_last_error(e)); return rc; }
  } else {
    MK_BGZF_HIP(F.setup(occ, qmin));
    MK_BGZF_HIP(F.reserve(S, MK_FQ_CARRY + max_text, rows_bytes));
  }

  /* chunk k: file -> pinned staging -> device (copy stream), inflate behind it on the engine's stream */
  auto queue_inflate = [&](size_t k) -> int {
    const mk_bgzf_chunk &c = chunks[k];
    const int s = (int)(k & 1u);
    const double t0 = mk_now_s();
    const uint64_t in_bytes = c.in1 - c.in0, tab_at = (in_bytes + 15u) & ~(uint64_t)15u;
    for (uint64_t got = 0; got < in_bytes;) {
      const ssize_t r = pread(fd, R.h_stage[s] + got, in_bytes - got, (off_t)(c.in0 + got));
      if (r <= 0) { snprintf(mk_bgzf_err, sizeof mk_bgzf_err, "reading the file failed"); (void)hipStreamSynchronize(S); (void)hipStreamSynchronize(R.copy); return MK_ERR_IO; }
      got += (uint64_t)r;
    }
    mk_infl_blk *tab = (mk_infl_blk *)(R.h_stage[s] + tab_at);
    for (uint64_t i = c.b0; i < c.b1; i++) {
      const mk_bgzf_block &b = R.blocks[i];
      tab[i - c.b0] = mk_infl_blk{(uint32_t)(b.in_off - c.in0 + b.pay_off), b.pay_len, (uint32_t)(MK_FQ_CARRY + (b.out_off - R.blocks[c.b0].out_off)), b.isize, b.crc32};
    }
    stats.t_read_s += mk_now_s() - t0;
    const uint32_t nb = (uint32_t)(c.b1 - c.b0);
    MK_BGZF_HIP(hipMemcpyAsync(R.d_comp[s], R.h_stage[s], tab_at + nb * sizeof(mk_infl_blk), hipMemcpyHostToDevice, R.copy));
    MK_BGZF_HIP(hipEventRecord(R.ev_up[s], R.copy));
    MK_BGZF_HIP(hipStreamWaitEvent(S, R.ev_up[s], 0));
    MK_BGZF_HIP(hipEventRecord(R.ev_i[s][0], S));
    MK_BGZF_HIP(mk_launch_inflate(S, R.d_comp[s], (const mk_infl_blk *)(R.d_comp[s] + tab_at), nb, R.d_text[s], R.d_status[s]));
    MK_BGZF_HIP(hipEventRecord(R.ev_i[s][1], S));
    return MK_OK;
  };

  /* the long sink's push: occ chooses fastq2co's rule with its mask */
  auto long_push = [&](const uint8_t *d, uint64_t n, int fin) -> int {
    return occ ? mk_sketch_push_fastq_long_q_device(e, d, n, fin, qmin) : mk_sketch_push_fastq_long_device(e, d, n, fin);
  };
  if (lng && chunks.empty()) { /* (a file without a member has no text) */
    if (final_in && (rc = long_push(nullptr, 0, 1))) { snprintf(mk_bgzf_err, sizeof mk_bgzf_err, "%s", mk_last_error(e)); return rc; }
    stats.comp_bytes = size; stats.t_total_s = mk_now_s() - t_begin;
    if (st) *st = stats;
    return MK_OK;
  }
  rc = queue_inflate(0);
  if (rc) return rc;
  uint32_t carry = 0;
  mk_fq_handed out{};
  auto push = [&](const uint8_t *d_rows, uint32_t stride, uint32_t nrows) -> int {
    return mk_sketch_push_reads_device(e, d_rows, stride, nrows, first_ordinal + stats.rows + out.rows);
  };
  float ms = 0.f, rows_ms = 0.f;
  int result = MK_OK;
  for (size_t k = 0; k < chunks.size(); k++) {
    const mk_bgzf_chunk &c = chunks[k];
    const int s = (int)(k & 1u), final = k + 1 == chunks.size();
    if (lng) {
      hipLaunchKernelGGL(mk_bgzf_bad_kernel, dim3(1), dim3(1024), 0, S, (const uint32_t *)R.d_status[s], (uint32_t)(c.b1 - c.b0), R.d_bad);
      MK_BGZF_HIP(hipGetLastError());
      MK_BGZF_HIP(hipMemcpyAsync(R.h_bad, R.d_bad, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, S));
      MK_BGZF_HIP(hipEventRecord(R.ev_bad, S));
      if (!final) { /* the next chunk's bytes travel beside this one's framing and scan; its text buffer was chunk k - 1's, which the engine has copied out of on S */
        rc = queue_inflate(k + 1);
        if (rc) return rc;
      }
      MK_BGZF_HIP(hipEventSynchronize(R.ev_bad)); /* the one wait per chunk */
      MK_BGZF_HIP(hipEventElapsedTime(&ms, R.ev_i[s][0], R.ev_i[s][1]));
      stats.inflate_ms += ms;
      if (R.h_bad[0] != 0xffffffffu) {
        stats.bad_block = (int64_t)(c.b0 + R.h_bad[0]);
        stats.bad_status = (int32_t)R.h_bad[1];
        snprintf(mk_bgzf_err, sizeof mk_bgzf_err, "BGZF block %llu: %s", (unsigned long long)stats.bad_block, mk_inflate_status_text(stats.bad_status));
        result = MK_ERR_FORMAT;
        break;
      }
      rc = long_push(R.d_text[s] + MK_FQ_CARRY, c.text, final_in && final);
      if (rc) { (void)hipStreamSynchronize(S); (void)hipStreamSynchronize(R.copy); snprintf(mk_bgzf_err, sizeof mk_bgzf_err, "%s", mk_last_error(e)); return rc; }
      continue;
    }
    const uint32_t t0 = MK_FQ_CARRY - carry, e1 = MK_FQ_CARRY + (uint32_t)c.text;
    MK_BGZF_HIP(F.count(S, R.d_text[s], t0, e1, final, R.d_status[s], (uint32_t)(c.b1 - c.b0)));
    if (!final) { /* the next chunk's bytes travel and inflate beside this one's framing and scan (its slots were chunk k - 1's, whose read-back has been waited for) */
      rc = queue_inflate(k + 1);
      if (rc) return rc;
    }
    mk_fq_chunk q;
    MK_BGZF_HIP(F.result(stats.rows, &q)); /* the one wait per chunk: rows, longest line, consumed, status */
    MK_BGZF_HIP(hipEventElapsedTime(&ms, R.ev_i[s][0], R.ev_i[s][1]));
    stats.inflate_ms += ms;
    MK_BGZF_HIP(F.times(&ms, &rows_ms)); /* (the rows: the chunk before) */
    stats.frame_ms += ms + rows_ms;
    if (q.r.bad_block != 0xffffffffu) {
      stats.bad_block = (int64_t)(c.b0 + q.r.bad_block);
      stats.bad_status = (int32_t)q.r.bad_status;
      snprintf(mk_bgzf_err, sizeof mk_bgzf_err, "BGZF block %llu: %s", (unsigned long long)stats.bad_block, mk_inflate_status_text(stats.bad_status));
      result = MK_ERR_FORMAT;
      break;
    }
    if (q.long_line) {
      snprintf(mk_bgzf_err, sizeof mk_bgzf_err, "a FASTQ line of 4095 characters or more");
      result = MK_ERR_FORMAT;
      break;
    }
    MK_BGZF_HIP(F.rows(S, q, push, &out));
    if (out.push_rc) { (void)hipStreamSynchronize(S); (void)hipStreamSynchronize(R.copy); snprintf(mk_bgzf_err, sizeof mk_bgzf_err, "%s", mk_last_error(e)); return out.push_rc; }
    stats.rows += out.rows;
    carry = out.carry;
    if (!final && carry) {
      hipLaunchKernelGGL(mk_fq_carry_kernel, dim3((carry + 255u) / 256u), dim3(256), 0, S, (const uint8_t *)R.d_text[s], t0 + q.r.consumed, R.d_text[s ^ 1], MK_FQ_CARRY - carry, carry);
      MK_BGZF_HIP(hipGetLastError());
    }
  }
  MK_BGZF_HIP(hipStreamSynchronize(S));
  MK_BGZF_HIP(hipStreamSynchronize(R.copy));
  if (lng) {
    double frame1 = frame0;
    (void)mk_sketch_fastq_long_frame_ms(e, &frame1);
    stats.frame_ms = frame1 - frame0;
  } else {
    MK_BGZF_HIP(F.times(&ms, &rows_ms));
    stats.frame_ms += rows_ms;
  }
  stats.blocks = nblocks; stats.chunks = chunks.size(); stats.comp_bytes = size; stats.text_bytes = total;
  stats.t_total_s = mk_now_s() - t_begin;
  if (st) *st = stats;
  return result;
}

extern "C" int mk_sketch_push_bgzf(mk_engine *e, int fd, size_t size, const mk_bgzf_opts *o, uint64_t first_ordinal, mk_bgzf_stats *st) {
  return mk_push_bgzf(e, fd, size, o, false, 0, first_ordinal, st);
}

extern "C" int mk_sketch_push_bgzf_q(mk_engine *e, int fd, size_t size, const mk_bgzf_opts *o, int32_t qmin, uint64_t first_ordinal, mk_bgzf_stats *st) {
  return mk_push_bgzf(e, fd, size, o, true, qmin, first_ordinal, st);
}

extern "C" int mk_sketch_push_bgzf_long(mk_engine *e, int fd, size_t size, const mk_bgzf_opts *o, int final, mk_bgzf_stats *st) {
  return mk_push_bgzf(e, fd, size, o, false, 0, 0, st, true, final);
}

extern "C" int mk_sketch_push_bgzf_long_q(mk_engine *e, int fd, size_t size, const mk_bgzf_opts *o, int32_t qmin, int final, mk_bgzf_stats *st) {
  return mk_push_bgzf(e, fd, size, o, true, qmin, 0, st, true, final);
}

extern "C" const char *mk_bgzf_last_error(void) { return mk_bgzf_err; }

#include "mk_gunzip.hip.h"
#include "mk_gunzip_batch.hip.h"
