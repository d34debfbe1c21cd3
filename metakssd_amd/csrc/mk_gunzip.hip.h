/* mk_gunzip.hip.h -- ONE gzip member of any size inflated by many wavefronts (part of mk_inflate.hip, which includes it last; gfx950,
 * wave64, hand-written).  The known two-pass method (pugz, rapidgzip) around this file's decoder:
 *
 *   mk_gun_find_kernel     one wave per span of S compressed bytes: the first bit of the span at which a NON-FINAL DYNAMIC block
 *                          header is valid.  64 lanes test 64 consecutive bit offsets with the cheap tests (the three header bits,
 *                          HLIT and HDIST <= 29, Kraft's sum over the 3-bit code length lengths, all bits inside the payload); a
 *                          survivor is tested by the whole wave with the decoder's own header walk and table builder: a complete
 *                          code length code, lengths without overrun, a code for symbol 256, a complete literal/length code, a
 *                          distance code the decoder accepts.  Stored and fixed blocks are never candidates.
 *   mk_gun_decode_kernel   one wave per piece (span 0 and every candidate start one): mk_inflate_kernel's decode with 16-bit output.
 *                          A literal is its byte; a match source inside the piece is copied symbol by symbol; a source in front of
 *                          the piece's first symbol is the marker 0x8000 | (32768 + source), source < 0.  In front of every block
 *                          header the bit position is held against the next piece's start: equal stops the piece, past it is
 *                          MK_INFL_MISSED.  More symbols than the piece's capacity: MK_INFL_CAPACITY.
 *   mk_gun_chain_kernel    one workgroup, pieces in order: W(c), the last 32 KiB of the text up to piece c's end, from W(c - 1) and
 *                          piece c's symbols.  All of a batch's windows are kept: W(c - 1) is what piece c's markers index.
 *   mk_gun_resolve_kernel  all pieces at once: text[off(c) + i] = sym < 0x8000 ? sym : W(c - 1)[sym & 0x7fff]
 * The text's CRC32 is mk_crc32_files_kernel's and the combine kernel's over segments of at most 1 GiB, carried from batch to batch
 * on the host.  Safety: the finder and the decode load inside the uploaded payload and the zeroed slack behind it, a piece stores
 * inside its cap symbols, the chain inside its windows, the resolve inside the sum of the lengths the decode reported; every loop
 * consumes input bits or produces output symbols and is bounded by the two sizes.  Bound of each kernel: DESIGN.md 4.14.
 *
 * MK_GUNZIP_REPAIR: the finder validates a header and nothing behind it, so an image of one inside compressed data
 * is a piece start that is none.  Without the flag that is MK_INFL_MISSED; with it the host repairs the table after the decode
 * launch, by an exact rule.  A piece whose start is a true block start decodes true text for as long as it runs, so when it runs
 * past the next start it has proved that start false and stands, at the block header where it noticed, on a true start: `stop`.
 * The walk goes over the batch's pieces in stream order and carries "this piece's start is confirmed" (the stream's first piece
 * is; a piece is when the one in front is and stopped at its start with MK_INFL_OK; a batch's first piece through the last of the
 * batch in front).  For a confirmed piece:
 *   MK_INFL_OK        the next piece is confirmed
 *   MK_INFL_MISSED    every start in [end, stop) leaves starts / kinds -- those of later batches too, which are found first; stop
 *                     becomes a block-kind start unless it is one; the piece is MK_INFL_OK with end = stop and the symbols it gave;
 *                     what the dropped pieces reported is discarded
 *   MK_INFL_CAPACITY  not the stream's last piece: the decode cannot say where it was (a stored block refuses at its header), so
 *                     the next start is dropped and the piece decoded again from its start with R * (the merged range), at most
 *                     MK_GUNZIP_REPAIR_MERGES times; a merge with a true start is still correct, the bound only keeps one wave
 *                     from being handed the whole file
 *   anything else     is the call's status.  A status of an unconfirmed piece means nothing until it is confirmed or dropped.
 * A new or re-sized piece is decoded by one launch of mk_gun_decode_kernel<false> over a table of that piece alone, its symbols at
 * the tail of the symbol buffer (which grows with its content kept); then the walk goes on from it.  Every launch follows a dropped
 * start, so there are fewer launches than starts.  A piece whose status came from compressed bytes that had not been uploaded yet
 * (stop behind them) is decoded again once more have arrived.  Chain, resolve, CRC and sink run once, over the final table; a
 * resumed piece at or behind the batch's bit_end is the next batch's.  Safety: a table entry of this path has the cap and symbol
 * range the first launch's entries have (R * covered bytes, inside nsyms <= syms_cap), so the kernel's bounds hold unchanged.
 * The two further MK_INFL_MISSED sites of the <true> decode are not repaired: both flags together are MK_ERR_ARG.
 *
 * MK_GUNZIP_MEMBERS: the payload may hold further members, each behind the trailer of the one in front.  The
 * <true> instances of finder and decode are for it; the <false> ones are the kernels described above, unchanged.
 *   finder     a second rule at byte-aligned lanes: a gzip header of at most MK_GUN_HDR_MAX bytes and behind it a dynamic block
 *              header, final or not, that passes the block rule's validation.  The kind travels in bit 63 of cand[].
 *   decode     behind a final block in front of the payload's end: the trailer into a member record {symbols so far, CRC32,
 *              ISIZE}, a stop where the next piece starts at the header behind it, else the header walk (MK_INFL_BAD_MEMBER when
 *              there is none) and on.  Distances are held against the member's start wherever the piece has seen it.
 *   check      mk_gun_members_kernel turns the records into text positions of the batch; the CRC table has a segment per member
 *              range, and the host holds every member's length and CRC32 against its own trailer.
 * Safety: trailer and header bytes are loaded below pay_len only, the FNAME and FCOMMENT walks compare every address with the
 * payload's end before the load; a piece's records stay inside its mem_cap slots, the count tested before every store (a member
 * takes 20 compressed bytes, the slots are counted from that, so the test never fails); every loop consumes input -- a boundary 18
 * bytes, a turn of the name walk 64; MK_POISON covers the record buffers, of which only entries below the count are read; plain
 * C++ and vector stores only. */

#include <algorithm>

namespace {

#define MK_GUN_WINDOW 32768u
#define MK_GUN_NONE (~(uint64_t)0)
#define MK_GUN_SLACK 64u              /* zeroed bytes behind the file's last byte on the device */
#define MK_GUN_SLICE ((uint64_t)128 << 20) /* text bytes one framing pass takes */
#define MK_GUN_CRC_SEG ((uint64_t)1 << 30)

typedef mk_bits_t<true> mk_zbits;

struct mk_gun_piece { /* the device's table, one entry a piece of the batch */
  uint64_t start;    /* bit in the payload */
  uint64_t end;      /* the next piece's start; MK_GUN_NONE: the stream's last piece */
  uint64_t sym_off;  /* its symbols in the batch's symbol buffer */
  uint64_t text_off; /* its text in the batch's text: the host's prefix sum over `len` */
  uint32_t cap;      /* symbols it may give */
  uint32_t first;    /* the stream's first piece: nothing lies in front of it */
  uint32_t status, len; /* left by the decode */
  uint64_t stop;     /* the bit the decode stopped at */
  /* MK_GUNZIP_MEMBERS (zeros without it) */
  uint32_t kind;     /* MK_GUN_K_* */
  uint32_t mem_cap;  /* member records it may write: (bytes covered) / 20 + 2 */
  uint64_t mem_off;  /* its records in the batch's record buffer */
  uint32_t nmem;     /* left by the decode: members that ended in the piece */
  uint32_t rec_off;  /* the host's prefix sum over nmem: its records in the batch's dense list */
};
#define MK_GUN_K_MEMBER 1u      /* the piece starts at a member's header */
#define MK_GUN_K_NEXT_MEMBER 2u /* the next piece does */
#define MK_GUN_HDR_MAX 4096u    /* the longest member header the finder walks; the decode walks any */

struct mk_gun_member { /* a member's end as the decode met it */
  uint32_t at;       /* decode: symbols of the piece in front of the end; dense list: text bytes of the batch in front of it */
  uint32_t crc32, isize; /* its trailer */
  uint32_t pad;
};

__device__ __forceinline__ uint64_t mk_uni64(uint64_t v) { return (uint64_t)mk_uni((uint32_t)(v >> 32)) << 32 | mk_uni((uint32_t)v); }

/* The first payload byte behind the member header at payload byte q, by the whole wave and the same in every lane.  0: no header
 * there with a payload byte behind it -- a wrong magic, CM != 8, reserved FLG bits, a field that runs past the payload -- or one
 * longer than `most` bytes.  FHCRC is skipped, not verified.  Loads: payload bytes below pay_len; each turn of the FNAME / FCOMMENT
 * walk takes 64 of them. */
__device__ uint64_t mk_gun_header_end(const uint8_t *__restrict__ comp, uint32_t shift, uint64_t pay_len, uint64_t q, uint64_t most, uint32_t lane) {
  if (q >= pay_len || pay_len - q < 10u) return 0;
  const uint8_t *p = comp + shift;
  const uint32_t w = mk_uni((uint32_t)p[q] | (uint32_t)p[q + 1u] << 8 | (uint32_t)p[q + 2u] << 16 | (uint32_t)p[q + 3u] << 24);
  if ((w & 0xe0ffffffu) != 0x00088b1fu) return 0;
  const uint32_t flg = w >> 24;
  const uint64_t lim = pay_len - q < most ? pay_len : q + most; /* the header ends at or in front of this byte */
  uint64_t at = q + 10u;
  if (at > lim) return 0;
  if (flg & 4u) { /* FEXTRA */
    if (lim - at < 2u) return 0;
    const uint32_t xlen = mk_uni((uint32_t)p[at] | (uint32_t)p[at + 1u] << 8);
    at += 2u;
    if (lim - at < xlen) return 0;
    at += xlen;
  }
  for (uint32_t bit = 8u; bit <= 16u; bit <<= 1) { /* FNAME, FCOMMENT: zero-terminated */
    if (!(flg & bit)) continue;
    bool hit = false;
    while (at < lim) {
      const uint64_t a = at + lane;
      const uint64_t m = __ballot(a < lim && p[a] == 0);
      if (m) { at += (uint64_t)__builtin_ctzll(m) + 1u; hit = true; break; }
      at += 64u;
    }
    if (!hit) return 0;
  }
  if (flg & 2u) { /* FHCRC */
    if (lim - at < 2u) return 0;
    at += 2u;
  }
  return at < pay_len ? at : 0;
}

/* the dynamic block header behind BTYPE (b refilled): HLIT, HDIST, HCLEN, the code length code, the lengths into L.lens[0, nl + nd)
 * -> MK_INFL_*, the same in every lane */
template <class B>
__device__ uint32_t mk_dyn_lengths(B &b, mk_infl_lds &L, uint32_t lane, uint32_t &nl, uint32_t &nd) {
  nl = b.get(5) + 257u;
  nd = b.get(5) + 1u;
  const uint32_t nc = b.get(4) + 4u;
  if (nl > 286u || nd > 30u) return MK_INFL_BAD_LENGTHS;
  if (lane < 19u) L.lens[320u + lane] = 0;
  mk_lds_fence();
  for (uint32_t i = 0; i < nc; i++) {
    b.refill();
    const uint32_t v = b.get(3);
    if (lane == 0u) L.lens[320u + mk_clorder[i]] = (uint8_t)v;
  }
  mk_lds_fence();
  if (mk_build(L.lens + 320, 19u, L.dist_cnt, L.dist_sym, L.dist_tab, 7u, false, lane)) return MK_INFL_BAD_CODE;
  uint32_t idx = 0, prev = 0;
  while (idx < nl + nd) {
    b.refill();
    if (b.past_end()) return MK_INFL_INPUT;
    const int s = mk_decode(b, L.dist_tab, 7u, L.dist_cnt, L.dist_sym);
    if (s < 0) return MK_INFL_BAD_CODE;
    if (s < 16) {
      if (lane == 0u) L.lens[idx] = (uint8_t)s;
      prev = (uint32_t)s;
      idx++;
      continue;
    }
    uint32_t rep, val = 0;
    if (s == 16) {
      if (idx == 0u) return MK_INFL_BAD_LENGTHS;
      val = prev;
      rep = 3u + b.get(2);
    } else if (s == 17) rep = 3u + b.get(3);
    else rep = 11u + b.get(7);
    if (idx + rep > nl + nd) return MK_INFL_BAD_LENGTHS;
    for (uint32_t i = lane; i < rep; i += 64u) L.lens[idx + i] = (uint8_t)val;
    prev = val;
    idx += rep;
  }
  mk_lds_fence();
  if (L.lens[256] == 0) return MK_INFL_BAD_LENGTHS;
  return MK_INFL_OK;
}

/* b at bit `bit` of the payload; comp is 16-byte aligned and holds the payload from comp + shift on.  Returns 8 * (the byte b's
 * coordinates start at, in the payload's): payload bit = b.bitpos() + that */
__device__ __forceinline__ int64_t mk_gun_seek(mk_zbits &b, const uint8_t *comp, uint32_t shift, uint64_t pay_len, uint64_t bit) {
  const uint64_t base_off = ((uint64_t)shift + (bit >> 3)) & ~(uint64_t)15u;
  const uint64_t end = (uint64_t)shift + pay_len - base_off;
  b.base = comp + base_off;
  b.end = end < 0xfffffff0ull ? (uint32_t)end : 0xfffffff0u; /* (the host gives no piece 2 GiB to cover) */
  b.seek((uint32_t)((uint64_t)shift + (bit >> 3) - base_off));
  b.get((uint32_t)bit & 7u);
  return 8 * ((int64_t)base_off - (int64_t)shift);
}

/* The finder's rule over the bits [lo, hi) of one payload, hi <= 8 * pay_len, by one wave with its LDS L: the lowest position, the
 * same in every lane, MK_GUN_NONE when there is none (mk_gunzip_batch.hip.h calls it with the payload of the file a span belongs
 * to).  MEMBERS: the lowest position of
 * either kind -- a block start as ever, or 8 * (a byte q at which a member header of at most MK_GUN_HDR_MAX bytes stands and, at the
 * first bit behind it, a dynamic block header, final or not, that passes the same validation), with MK_GUNZIP_PIECE_MEMBER set.
 * The two never meet at one bit: 0x1f has BFINAL set. */
template <bool MEMBERS>
__device__ __forceinline__ uint64_t mk_gun_find_span(const uint8_t *__restrict__ comp, uint32_t shift, uint64_t pay_len, uint64_t lo, uint64_t hi,
                                                     mk_infl_lds &L, uint32_t lane) {
  const uint64_t nbits = 8u * pay_len;
  const uint32_t *words = (const uint32_t *)comp;
  uint64_t found = MK_GUN_NONE;
  for (uint64_t p0 = lo; p0 < hi && found == MK_GUN_NONE; p0 += 64u) {
    const uint64_t p = p0 + lane;
    bool ok = false, okm = false;
    if (p < hi) { /* 128 bits from bit p on: four aligned words, inside the payload, its trailer and the slack */
      const uint64_t q = p + 8u * shift;
      const uint64_t w = q >> 5;
      const uint32_t sh = (uint32_t)q & 31u;
      const uint64_t a = (uint64_t)words[w] | (uint64_t)words[w + 1u] << 32, bq = (uint64_t)words[w + 2u] | (uint64_t)words[w + 3u] << 32;
      const uint64_t v0 = sh ? a >> sh | bq << (64u - sh) : a, v1 = bq >> sh;
      const uint32_t h = (uint32_t)v0;
      const uint32_t nc = ((h >> 13) & 15u) + 4u;
      if ((h & 7u) == 4u && ((h >> 3) & 31u) <= 29u && ((h >> 8) & 31u) <= 29u && p + 17u + 3u * nc <= nbits) {
        const uint64_t t0 = v0 >> 17, t1 = v0 >> 62 | v1 << 2; /* triples 0..14, triples 15..18 */
        uint32_t kraft = 0;
        for (uint32_t k = 0; k < 19u; k++) {
          const uint32_t n = (uint32_t)(k < 15u ? t0 >> (3u * k) : t1 >> (3u * (k - 15u))) & 7u;
          if (k < nc && n) kraft += 128u >> n;
        }
        ok = kraft == 128u;
      }
      if (MEMBERS) okm = ((uint32_t)p & 7u) == 0u && (h & 0xe0ffffffu) == 0x00088b1fu && p + 32u <= nbits;
    }
    const uint64_t mm = MEMBERS ? __ballot(okm) : 0ull;
    uint64_t m = __ballot(ok) | mm;
    while (m && found == MK_GUN_NONE) { /* the survivors, lowest bit first, each by the whole wave */
      const uint32_t at = (uint32_t)__builtin_ctzll(m);
      const uint64_t cp = p0 + (uint64_t)at;
      const bool member = MEMBERS && ((mm >> at) & 1ull);
      m &= m - 1ull;
      uint64_t hb = cp; /* where the block header stands */
      if (member) {
        const uint64_t he = mk_gun_header_end(comp, shift, pay_len, cp >> 3, MK_GUN_HDR_MAX, lane);
        if (!he) continue;
        hb = 8u * he;
      }
      mk_zbits b;
      b.win = L.win;
      b.lane = lane;
      mk_gun_seek(b, comp, shift, pay_len, hb);
      b.refill();
      if (member) {
        b.get(1);
        if (b.get(2) != 2u) continue;
      } else b.get(3);
      uint32_t nl = 0, nd = 0;
      if (mk_dyn_lengths(b, L, lane, nl, nd) || b.past_end()) continue;
      if (mk_build(L.lens, nl, L.lit_cnt, L.lit_sym, L.lit_tab, MK_INFL_LBITS, false, lane)) continue;
      if (mk_build(L.lens + nl, nd, L.dist_cnt, L.dist_sym, L.dist_tab, MK_INFL_DBITS, true, lane)) continue;
      found = member ? cp | MK_GUNZIP_PIECE_MEMBER : cp;
    }
  }
  return found;
}

/* cand[i]: the candidate of span span0 + i (span0 >= 1), MK_GUN_NONE when the span has none */
template <bool MEMBERS>
__global__ void __launch_bounds__(64 * MK_INFL_WAVES) mk_gun_find_kernel(const uint8_t *__restrict__ comp, uint32_t shift, uint64_t pay_len, uint32_t S,
                                                                          uint64_t span0, uint32_t nspans, uint64_t *cand) {
  __shared__ mk_infl_lds lds_all[MK_INFL_WAVES];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x * MK_INFL_WAVES + wave;
  if (i >= nspans) return;
  const uint64_t c = span0 + i, nbits = 8u * pay_len;
  const uint64_t lo = 8u * c * S, hi = 8u * (c + 1u) * S < nbits ? 8u * (c + 1u) * S : nbits;
  const uint64_t found = mk_gun_find_span<MEMBERS>(comp, shift, pay_len, lo, hi, lds_all[wave], lane);
  if (lane == 0u) cand[i] = found;
}

/* MEMBERS: behind a final block that ends in front of the payload's end the wave reads the member's trailer into a member record,
 * stops where the next piece starts at the header behind it, and otherwise walks that header and decodes on (4.15). */
template <bool MEMBERS>
__device__ __forceinline__ void mk_gun_decode_piece(const uint8_t *__restrict__ comp, uint32_t shift, uint64_t pay_len, mk_gun_piece *pieces, uint32_t k,
                                                    uint16_t *syms, mk_gun_member *mems, mk_infl_lds &L, uint32_t lane) {
  const uint64_t start = mk_uni64(pieces[k].start), end_bit = mk_uni64(pieces[k].end);
  const uint32_t cap = mk_uni(pieces[k].cap), back = mk_uni(pieces[k].first) ? 0u : MK_GUN_WINDOW;
  const bool last_piece = end_bit == MK_GUN_NONE;
  uint16_t *out = syms + mk_uni64(pieces[k].sym_off);
  const uint32_t kind = MEMBERS ? mk_uni(pieces[k].kind) : 0u, mem_cap = MEMBERS ? mk_uni(pieces[k].mem_cap) : 0u;
  const bool next_member = (kind & MK_GUN_K_NEXT_MEMBER) != 0u;
  mk_gun_member *rec = MEMBERS ? mems + mk_uni64(pieces[k].mem_off) : nullptr;
  bool seen = back == 0u || (kind & MK_GUN_K_MEMBER); /* the piece has seen the start of the member it is in ... */
  uint32_t mstart = 0, nmem = 0;                      /* ... at this symbol */
  uint32_t st = MK_INFL_OK, pos = 0, nlit = 0, synced = 0, lit = 0;
  uint64_t from_bit = start, stop_bit = MK_GUN_NONE;
  if (MEMBERS && (kind & MK_GUN_K_MEMBER)) { /* a member-start piece begins by walking its header */
    const uint64_t he = mk_gun_header_end(comp, shift, pay_len, start >> 3, ~(uint64_t)0, lane);
    if (he) from_bit = 8u * he;
    else st = MK_INFL_BAD_MEMBER;
  }
  mk_zbits b;
  b.win = L.win;
  b.lane = lane;
  int64_t bit0 = mk_gun_seek(b, comp, shift, pay_len, from_bit);

  auto flush = [&]() { /* pending literals -> one store (they were counted against cap when they came) */
    if (nlit) {
      if (lane < nlit) out[pos + lane] = (uint16_t)lit;
      pos += nlit;
      nlit = 0;
    }
  };
  while (!st) {
    b.refill();
    if (!last_piece) {
      const uint64_t at = (uint64_t)((int64_t)b.bitpos() + bit0);
      if (at == end_bit && !(MEMBERS && next_member)) break;
      if (at > end_bit) { st = MK_INFL_MISSED; break; }
    }
    if (b.past_end()) { st = MK_INFL_INPUT; break; }
    const uint32_t last = b.get(1), type = b.get(2);
    if (type == 0u) {
      b.get(b.cnt & 7u);
      b.refill();
      const uint32_t len = b.get(16), nlen = b.get(16);
      if ((len ^ nlen) != 0xffffu) { st = MK_INFL_BAD_BLOCK; break; }
      const uint32_t a0 = (uint32_t)(b.bitpos() >> 3);
      if (b.past_end() || a0 + len > b.end) { st = MK_INFL_INPUT; break; }
      if (pos + nlit + len > cap) { st = MK_INFL_CAPACITY; break; }
      flush();
      for (uint32_t i = lane; i < len; i += 64u) out[pos + i] = (uint16_t)b.base[a0 + i];
      pos += len;
      b.seek(a0 + len);
    } else if (type == 3u) {
      st = MK_INFL_BAD_BLOCK;
      break;
    } else {
      uint32_t nl = 288u, nd = 32u;
      if (type == 1u) {
        for (uint32_t i = lane; i < 320u; i += 64u) L.lens[i] = (uint8_t)(i < 144u ? 8u : i < 256u ? 9u : i < 280u ? 7u : i < 288u ? 8u : 5u);
        mk_lds_fence();
      } else {
        st = mk_dyn_lengths(b, L, lane, nl, nd);
        if (st) break;
      }
      if (mk_build(L.lens, nl, L.lit_cnt, L.lit_sym, L.lit_tab, MK_INFL_LBITS, true, lane) ||
          mk_build(L.lens + nl, nd, L.dist_cnt, L.dist_sym, L.dist_tab, MK_INFL_DBITS, true, lane)) { st = MK_INFL_BAD_CODE; break; }
      for (;;) { /* the tokens of this block: each takes at least one bit of input */
        b.refill();
        if (b.past_end()) { st = MK_INFL_INPUT; break; }
        int s = mk_decode(b, L.lit_tab, MK_INFL_LBITS, L.lit_cnt, L.lit_sym);
        if (s < 0) { st = MK_INFL_BAD_CODE; break; }
        if (s < 256) {
          if (pos + nlit + 1u > cap) { st = MK_INFL_CAPACITY; break; }
          if (lane == nlit) lit = (uint32_t)s;
          if (++nlit == 64u) flush();
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
        flush();
        if (dist > (MEMBERS && seen ? pos - mstart : pos + back)) { st = MK_INFL_BAD_DISTANCE; break; }
        if (pos + len > cap) { st = MK_INFL_CAPACITY; break; }
        const int32_t from = (int32_t)pos - (int32_t)dist; /* >= -32768; pos < 2^31 */
        if (from + (int32_t)(len < dist ? len : dist) > (int32_t)synced) { mk_store_fence(); synced = pos; } /* the source was written since the last wait */
        for (uint32_t i = lane; i < len; i += 64u) {
          const int32_t src = from + (int32_t)(dist >= len ? i : i % dist);
          out[pos + i] = src < 0 ? (uint16_t)(0x8000u | (uint32_t)((int32_t)MK_GUN_WINDOW + src)) : out[src];
        }
        pos += len;
      }
      if (st) break;
    }
    if (last) {
      if (b.past_end()) { st = MK_INFL_INPUT; break; }
      if (!MEMBERS) {
        if (!last_piece || (((uint64_t)((int64_t)b.bitpos() + bit0) + 7u) >> 3) < pay_len) st = MK_INFL_TRAILING;
        break;
      }
      /* the boundary: trailer, member record, the next header.  Every turn takes at least 8 + 10 bytes of input */
      const uint64_t p = ((uint64_t)((int64_t)b.bitpos() + bit0) + 7u) >> 3; /* <= pay_len: not past the end */
      if (p == pay_len) { /* the stream ends; the last trailer lies behind the payload */
        if (!last_piece) st = MK_INFL_MISSED; /* (the next piece's start was not met, and nothing is left) */
        break;
      }
      if (pay_len - p < 8u + 10u + 1u) { st = MK_INFL_BAD_MEMBER; break; }
      flush();
      if (nmem >= mem_cap) { st = MK_INFL_CAPACITY; break; } /* (cannot happen: a member takes 20 bytes, the host counted the slots from that) */
      {
        const uint8_t *t = comp + shift + p;
        const uint32_t crc = mk_uni((uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24);
        const uint32_t isz = mk_uni((uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24);
        if (lane == 0u) rec[nmem] = mk_gun_member{pos, crc, isz, 0u};
        nmem++;
      }
      const uint64_t q = p + 8u;
      if (!last_piece) {
        if (8u * q == end_bit && next_member) { stop_bit = 8u * q; break; }
        if (8u * q > end_bit) { st = MK_INFL_MISSED; break; }
      }
      const uint64_t he = mk_gun_header_end(comp, shift, pay_len, q, ~(uint64_t)0, lane);
      if (!he) { st = MK_INFL_BAD_MEMBER; break; }
      bit0 = mk_gun_seek(b, comp, shift, pay_len, 8u * he);
      seen = true;
      mstart = pos;
    }
  }
  flush();
  if (lane == 0u) {
    pieces[k].status = st;
    pieces[k].len = pos;
    pieces[k].stop = stop_bit != MK_GUN_NONE ? stop_bit : (uint64_t)((int64_t)b.bitpos() + bit0);
    if (MEMBERS) pieces[k].nmem = nmem;
  }
}

/* one wave per piece of ONE stream (mk_gunzip_batch.hip.h has the kernel for the pieces of many files) */
template <bool MEMBERS>
__global__ void __launch_bounds__(64 * MK_INFL_WAVES) mk_gun_decode_kernel(const uint8_t *__restrict__ comp, uint32_t shift, uint64_t pay_len,
                                                                            mk_gun_piece *pieces, uint32_t npieces, uint16_t *syms, mk_gun_member *mems) {
  __shared__ mk_infl_lds lds_all[MK_INFL_WAVES];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t k = blockIdx.x * MK_INFL_WAVES + wave;
  if (k >= npieces) return;
  mk_gun_decode_piece<MEMBERS>(comp, shift, pay_len, pieces, k, syms, mems, lds_all[wave], lane);
}

/* win: npieces + 1 windows of 32 KiB; window 0 is W of the piece in front of the batch, window c + 1 becomes W(piece c) */
__global__ void __launch_bounds__(1024) mk_gun_chain_kernel(const mk_gun_piece *__restrict__ pieces, uint32_t npieces, const uint16_t *__restrict__ syms, uint8_t *win) {
  const uint32_t t = threadIdx.x;
  for (uint32_t c = 0; c < npieces; c++) {
    const uint32_t n = pieces[c].len;
    const uint16_t *s = syms + pieces[c].sym_off;
    const uint8_t *wp = win + (uint64_t)c * MK_GUN_WINDOW;
    uint8_t *wn = win + (uint64_t)(c + 1u) * MK_GUN_WINDOW;
    const uint32_t keep = n < MK_GUN_WINDOW ? MK_GUN_WINDOW - n : 0u; /* bytes of W(c - 1) that stay */
    for (uint32_t j = t; j < MK_GUN_WINDOW; j += 1024u) {
      uint32_t v;
      if (j < keep) v = wp[j + n];
      else {
        const uint32_t sym = s[n - (MK_GUN_WINDOW - j)]; /* j >= keep: n + j >= 32768 */
        v = sym < 0x8000u ? sym : wp[sym & 0x7fffu];
      }
      wn[j] = (uint8_t)v;
    }
    __syncthreads(); /* the workgroup's stores to W(c) are visible to its loads in the next turn */
  }
}

/* blockIdx.y: the piece */
__global__ void __launch_bounds__(256) mk_gun_resolve_kernel(const mk_gun_piece *__restrict__ pieces, const uint16_t *__restrict__ syms,
                                                             const uint8_t *__restrict__ win, uint8_t *text) {
  const uint32_t c = blockIdx.y, n = pieces[c].len;
  const uint16_t *s = syms + pieces[c].sym_off;
  const uint8_t *w = win + (uint64_t)c * MK_GUN_WINDOW;
  uint8_t *out = text + pieces[c].text_off;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const uint32_t sym = s[i];
    out[i] = (uint8_t)(sym < 0x8000u ? sym : w[sym & 0x7fffu]);
  }
}

/* blockIdx.x: the piece.  Its member records, symbol positions, become text positions of the batch in the dense list the host reads
 * (nmem <= mem_cap and rec_off, the prefix sum over nmem, are the host's: it has checked the first and made the second) */
__global__ void __launch_bounds__(64) mk_gun_members_kernel(const mk_gun_piece *__restrict__ pieces, const mk_gun_member *__restrict__ mems, mk_gun_member *dense) {
  const mk_gun_piece &P = pieces[blockIdx.x];
  const uint32_t text0 = (uint32_t)(P.text_off - MK_FQ_CARRY);
  for (uint32_t i = threadIdx.x; i < P.nmem; i += 64u) {
    const mk_gun_member m = mems[P.mem_off + i];
    dense[P.rec_off + i] = mk_gun_member{text0 + m.at, m.crc32, m.isize, 0u};
  }
}

/* ---- host ------------------------------------------------------------------------------------------------------------------- */
static uint32_t mk_crc_mul_host(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
  }
  return p;
}
/* the CRC32 of A || B from the CRC32s of A and B and B's length */
static uint32_t mk_crc_concat(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  uint32_t p = 1u << 31, sq = 0x00800000u; /* x^0, x^8 */
  for (uint64_t n = len_b; n; n >>= 1) {
    if (n & 1u) p = mk_crc_mul_host(sq, p);
    sq = mk_crc_mul_host(sq, sq);
  }
  return mk_crc_mul_host(p, crc_a) ^ crc_b;
}

struct mk_gun_result {
  int32_t status = MK_INFL_OK;
  int64_t bad_piece = -1;
  uint64_t text_len = 0, npieces = 0, nbatches = 0, members = 0;
  uint64_t repairs = 0; /* MK_GUNZIP_REPAIR: piece starts dropped */
  double find_ms = 0, decode_ms = 0, resolve_ms = 0, t_read_s = 0;
};

struct mk_gun_run { /* everything the stream decode allocates, released on every way out */
  hipStream_t S = nullptr, copy = nullptr;
  uint8_t *h_stage[2] = {nullptr, nullptr}, *d_comp = nullptr, *d_win = nullptr, *d_wcarry = nullptr, *d_text = nullptr, *d_fcarry = nullptr; /* d_fcarry: mk_push_gzip's, FASTQ text between batches */
  uint64_t *d_cand = nullptr, *h_cand = nullptr;
  mk_gun_piece *d_pieces = nullptr, *h_pieces = nullptr;
  uint16_t *d_syms = nullptr;
  uint8_t *d_crctab = nullptr, *h_crctab = nullptr;
  uint32_t *d_crcwork = nullptr, *h_crc = nullptr;
  mk_gun_member *d_mems = nullptr, *d_dense = nullptr, *h_dense = nullptr;
  uint64_t mems_cap = 0, dense_cap = 0, hdense_cap = 0;
  uint64_t cand_cap = 0, hcand_cap = 0, pieces_cap = 0, hpieces_cap = 0, syms_cap = 0, win_cap = 0, text_cap = 0, crctab_cap = 0, hcrctab_cap = 0, crcwork_cap = 0, hcrc_cap = 0;
  hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_t[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  char err[256] = {0};
  ~mk_gun_run() {
    for (int s = 0; s < 2; s++) { if (h_stage[s]) (void)hipHostFree(h_stage[s]); if (ev_up[s]) (void)hipEventDestroy(ev_up[s]); }
    void *dev[] = {d_comp, d_win, d_wcarry, d_text, d_fcarry, d_cand, d_pieces, d_syms, d_crctab, d_crcwork, d_mems, d_dense};
    for (void *p : dev) (void)hipFree(p);
    void *pin[] = {h_cand, h_pieces, h_crctab, h_crc, h_dense};
    for (void *p : pin) if (p) (void)hipHostFree(p);
    for (hipEvent_t e : ev_t) if (e) (void)hipEventDestroy(e);
    if (copy) (void)hipStreamDestroy(copy);
  }
};

#define MK_GUN_HIP(call)                                                                                   \
  do {                                                                                                     \
    hipError_t _r = (call);                                                                                \
    if (_r != hipSuccess) {                                                                                \
      snprintf(R.err, sizeof R.err, "%s: %s", #call, hipGetErrorString(_r));                               \
      (void)hipStreamSynchronize(R.S);                                                                     \
      if (R.copy) (void)hipStreamSynchronize(R.copy);                                                      \
      return MK_ERR_HIP;                                                                                   \
    }                                                                                                      \
  } while (0)

struct mk_gun_geom { uint32_t S, ratio, batch; };
static mk_gun_geom mk_gun_geometry(const mk_gunzip_opts *o) {
  mk_gun_geom g;
  g.S = o && o->span_bytes ? o->span_bytes : 128u << 10;
  if (g.S < 64u) g.S = 64u;
  if (g.S > (1u << 30)) g.S = 1u << 30;
  g.ratio = o && o->ratio ? o->ratio : 16u;
  if (g.ratio > 65536u) g.ratio = 65536u;
  uint64_t most = ((uint64_t)1 << 31) / ((uint64_t)g.ratio * g.S); /* R * S * spans <= 2 GiB of text a batch */
  if (most < 1u) most = 1u;
  if (most > 32768u) most = 32768u; /* (a piece per span at most: the resolve grid's second dimension) */
  g.batch = o && o->batch_spans && o->batch_spans < most ? o->batch_spans : (uint32_t)most;
  return g;
}

/* The stream behind `info` of a file of `size` bytes that `read(offset, n, dst)` hands out, on R.S of the current device.  Batch
 * after batch sink(d_text, n, final) gets the resolved text: n bytes at d_text + MK_FQ_CARRY (a buffer of whole tiles with
 * MK_FQ_CARRY bytes of room in front), valid until it returns; it returns MK_OK or an error that ends the run.  pieces_out (may be
 * null): every piece decoded.  MK_OK with res.status set when the decode met a status; the trailer is checked behind the last batch. */
template <class Read, class Sink>
static int mk_gun_stream(mk_gun_run &R, uint64_t size, const mk_gzip_info &info, const mk_gunzip_opts *opts, Read read, Sink sink,
                         std::vector<mk_gunzip_piece> *pieces_out, mk_gun_result &res) {
  const mk_gun_geom G = mk_gun_geometry(opts);
  const uint64_t pay_len = info.pay_len, f0 = info.pay_off & ~(uint64_t)15u, total = size - f0; /* the device holds file bytes [f0, size) */
  const uint32_t shift = (uint32_t)(info.pay_off - f0), S = G.S;
  const bool members = opts && (opts->flags & MK_GUNZIP_MEMBERS);
  const bool repair = opts && (opts->flags & MK_GUNZIP_REPAIR);
  if (members && repair) { snprintf(R.err, sizeof R.err, "MK_GUNZIP_MEMBERS | MK_GUNZIP_REPAIR: member boundaries are not repaired yet"); return MK_ERR_ARG; }
  const uint64_t ahead = members ? 4096u + MK_GUN_HDR_MAX : 4096u; /* bytes behind a span the finder may read */
  if (!info.is_single || info.pay_off + pay_len + 8u != size || pay_len == 0) { snprintf(R.err, sizeof R.err, "not a single-member gzip file"); return MK_ERR_ARG; }
  const uint64_t NS = (pay_len + S - 1) / S, NB = (NS + G.batch - 1) / G.batch;
  const uint64_t stage_bytes = std::min<uint64_t>(std::max<uint64_t>((uint64_t)G.batch * S, 65536u), (uint64_t)32 << 20);
  MK_GUN_HIP(hipStreamCreateWithFlags(&R.copy, hipStreamNonBlocking));
  for (int s = 0; s < 2; s++) {
    if (s == 1 && total <= stage_bytes) break;
    MK_GUN_HIP(mk_pin_alloc(&R.h_stage[s], stage_bytes, hipHostMallocDefault));
    MK_GUN_HIP(hipEventCreateWithFlags(&R.ev_up[s], hipEventDisableTiming));
  }
  for (int k = 0; k < 6; k++) MK_GUN_HIP(hipEventCreate(&R.ev_t[k]));
  MK_GUN_HIP(mk_dev_alloc(&R.d_comp, total + MK_GUN_SLACK));
  MK_GUN_HIP(mk_dev_alloc(&R.d_wcarry, (size_t)MK_GUN_WINDOW));
  MK_GUN_HIP(hipMemsetAsync(R.d_comp + total, 0, MK_GUN_SLACK, R.S));
  MK_GUN_HIP(hipMemsetAsync(R.d_wcarry, 0, MK_GUN_WINDOW, R.S)); /* a reference in front of the text's first byte reads zeros: the CRC tells */

  uint64_t up = 0, nup = 0;
  /* file bytes [f0, f0 + upto) are on their way, and R.S waits for them */
  auto ensure_uploaded = [&](uint64_t upto) -> int {
    if (upto > total) upto = total;
    while (up < upto) {
      const int s = R.h_stage[1] ? (int)(nup & 1u) : 0;
      const uint64_t n = std::min<uint64_t>(stage_bytes, total - up);
      if (nup >= (R.h_stage[1] ? 2u : 1u)) MK_GUN_HIP(hipEventSynchronize(R.ev_up[s]));
      const double t0 = mk_now_s();
      const int rc = read(f0 + up, n, R.h_stage[s]);
      res.t_read_s += mk_now_s() - t0;
      if (rc) { snprintf(R.err, sizeof R.err, "reading the file failed"); (void)hipStreamSynchronize(R.S); (void)hipStreamSynchronize(R.copy); return rc; }
      MK_GUN_HIP(hipMemcpyAsync(R.d_comp + up, R.h_stage[s], n, hipMemcpyHostToDevice, R.copy));
      MK_GUN_HIP(hipEventRecord(R.ev_up[s], R.copy));
      MK_GUN_HIP(hipStreamWaitEvent(R.S, R.ev_up[s], 0));
      up += n;
      nup++;
    }
    return MK_OK;
  };

  std::vector<uint64_t> starts(1, 0); /* every piece start known so far, ascending */
  std::vector<uint8_t> kinds(1, 0);   /* ... and whether it is a member's header */
  uint64_t found = 0;                 /* batches whose candidates are known */
  auto find_batch = [&](uint64_t j) -> int {
    const uint64_t c0 = std::max<uint64_t>(1, j * G.batch), c1 = std::min<uint64_t>(NS, (j + 1) * G.batch);
    if (c1 <= c0) return MK_OK;
    const uint32_t n = (uint32_t)(c1 - c0);
    int rc = ensure_uploaded(shift + c1 * S + ahead); /* (a block header that starts in the span's last bits ends within 2.3 KB) */
    if (rc) return rc;
    MK_GUN_HIP(mk_grow(&R.d_cand, &R.cand_cap, n, false));
    MK_GUN_HIP(mk_grow(&R.h_cand, &R.hcand_cap, n, true));
    MK_GUN_HIP(hipEventRecord(R.ev_t[0], R.S));
    hipLaunchKernelGGL(members ? mk_gun_find_kernel<true> : mk_gun_find_kernel<false>, dim3((n + MK_INFL_WAVES - 1) / MK_INFL_WAVES), dim3(64 * MK_INFL_WAVES), 0, R.S,
                       (const uint8_t *)R.d_comp, shift, pay_len, S, c0, n, R.d_cand);
    MK_GUN_HIP(hipGetLastError());
    MK_GUN_HIP(hipEventRecord(R.ev_t[1], R.S));
    MK_GUN_HIP(hipMemcpyAsync(R.h_cand, R.d_cand, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, R.S));
    MK_GUN_HIP(hipStreamSynchronize(R.S));
    float ms = 0.f;
    MK_GUN_HIP(hipEventElapsedTime(&ms, R.ev_t[0], R.ev_t[1]));
    res.find_ms += ms;
    for (uint32_t i = 0; i < n; i++)
      if (R.h_cand[i] != MK_GUN_NONE) {
        starts.push_back(R.h_cand[i] & ~MK_GUNZIP_PIECE_MEMBER);
        kinds.push_back((uint8_t)(R.h_cand[i] >> 63));
      }
    return MK_OK;
  };

  uint64_t idx = 0; /* the first piece that has not been decoded */
  uint32_t crc = 0;      /* of the member in progress: its text up to the last batch's end ... */
  uint64_t crc_len = 0;  /* ... and that text's length */
  int32_t member_status = MK_INFL_OK; /* the first member in stream order whose check failed */
  std::vector<mk_gun_member> segs;    /* the CRC table's segments: at = 1 where one closes a member, whose trailer it then holds */
  for (uint64_t bt = 0; bt < NB && idx < starts.size(); bt++) {
    int rc;
    while (found < std::min<uint64_t>(NB, bt + 1)) { rc = find_batch(found++); if (rc) return rc; }
    const uint64_t bit_end = 8u * (bt + 1) * G.batch * S; /* pieces that start in front of this bit are the batch's */
    uint64_t idx_end = idx;
    while (idx_end < starts.size() && starts[idx_end] < bit_end) idx_end++;
    if (idx_end == idx) continue;
    while (idx_end == starts.size() && found < NB) { rc = find_batch(found++); if (rc) return rc; } /* where the batch's last piece ends */
    uint32_t np = (uint32_t)(idx_end - idx);
    bool final = idx_end == starts.size();
    MK_GUN_HIP(mk_grow(&R.h_pieces, &R.hpieces_cap, np, true));
    MK_GUN_HIP(mk_grow(&R.d_pieces, &R.pieces_cap, np, false));
    uint64_t nsyms = 0, nslots = 0;
    for (uint32_t k = 0; k < np; k++) {
      mk_gun_piece &P = R.h_pieces[k];
      memset(&P, 0, sizeof P);
      P.start = starts[idx + k];
      P.end = idx + k + 1 < starts.size() ? starts[idx + k + 1] : MK_GUN_NONE;
      const uint64_t covered = (P.end == MK_GUN_NONE ? pay_len : (P.end + 7u) >> 3) - (P.start >> 3);
      const uint64_t cap = (uint64_t)G.ratio * covered;
      if (cap >= ((uint64_t)1 << 31) || nsyms + cap >= ((uint64_t)1 << 32)) { /* no candidate for too long: one wave would decode gigabytes */
        (void)hipStreamSynchronize(R.S); (void)hipStreamSynchronize(R.copy);
        res.status = MK_INFL_CAPACITY; res.bad_piece = (int64_t)(idx + k);
        return MK_OK;
      }
      P.cap = (uint32_t)cap;
      P.first = idx + k == 0;
      P.sym_off = nsyms;
      nsyms += (cap + 7u) & ~(uint64_t)7u;
      if (members) { /* a member takes 20 compressed bytes at least */
        P.kind = (kinds[idx + k] ? MK_GUN_K_MEMBER : 0u) | (idx + k + 1 < starts.size() && kinds[idx + k + 1] ? MK_GUN_K_NEXT_MEMBER : 0u);
        P.mem_cap = (uint32_t)(covered / 20u + 2u);
        P.mem_off = nslots;
        nslots += P.mem_cap;
      }
    }
    if (members) MK_GUN_HIP(mk_grow(&R.d_mems, &R.mems_cap, nslots, false));
    MK_GUN_HIP(mk_grow(&R.d_syms, &R.syms_cap, nsyms, false));
    MK_GUN_HIP(mk_grow(&R.d_win, &R.win_cap, ((uint64_t)np + 1u) * MK_GUN_WINDOW, false));
    rc = ensure_uploaded(R.h_pieces[np - 1].end == MK_GUN_NONE ? total : shift + (R.h_pieces[np - 1].end >> 3) + 4096u);
    if (rc) return rc;
    MK_GUN_HIP(hipMemcpyAsync(R.d_pieces, R.h_pieces, (size_t)np * sizeof(mk_gun_piece), hipMemcpyHostToDevice, R.S));
    MK_GUN_HIP(hipEventRecord(R.ev_t[2], R.S));
    hipLaunchKernelGGL(members ? mk_gun_decode_kernel<true> : mk_gun_decode_kernel<false>, dim3((np + MK_INFL_WAVES - 1) / MK_INFL_WAVES), dim3(64 * MK_INFL_WAVES), 0, R.S,
                       (const uint8_t *)R.d_comp, shift, pay_len, R.d_pieces, np, R.d_syms, R.d_mems);
    MK_GUN_HIP(hipGetLastError());
    MK_GUN_HIP(hipEventRecord(R.ev_t[3], R.S));
    MK_GUN_HIP(hipMemcpyAsync(R.h_pieces, R.d_pieces, (size_t)np * sizeof(mk_gun_piece), hipMemcpyDeviceToHost, R.S));
    MK_GUN_HIP(hipStreamSynchronize(R.S));
    float ms = 0.f;
    MK_GUN_HIP(hipEventElapsedTime(&ms, R.ev_t[2], R.ev_t[3]));
    res.decode_ms += ms;
    res.nbatches++;
    if (repair) { /* the walk of the file's header comment.  T mirrors starts[idx, idx + T.size()) */
      std::vector<mk_gun_piece> T(R.h_pieces, R.h_pieces + np);
      std::vector<uint8_t> decoded(np, 1), merges(np, 0);
      std::vector<uint64_t> upl(np, up); /* file bytes the device held when the piece was decoded */
      auto drop = [&](uint32_t a, uint32_t b) { /* T[a, b) */
        T.erase(T.begin() + a, T.begin() + b);
        decoded.erase(decoded.begin() + a, decoded.begin() + b);
        merges.erase(merges.begin() + a, merges.begin() + b);
        upl.erase(upl.begin() + a, upl.begin() + b);
      };
      auto know_next = [&](uint64_t i) -> int { /* starts[i + 1] is known, or the stream has no start behind starts[i] */
        while (i + 1 >= starts.size() && found < NB) { const int r = find_batch(found++); if (r) return r; }
        return MK_OK;
      };
      uint32_t k = 0; /* pieces in front of T[k] are confirmed and final */
      for (;;) {
        int64_t redo = -1; /* the piece the next launch decodes */
        bool resize = false, stands = false;
        for (; k < T.size() && redo < 0 && !stands; k++) {
          mk_gun_piece &P = T[k];
          const uint64_t gi = idx + k;
          if (!decoded[k]) { redo = k; resize = true; break; }
          if (!P.status) continue;
          if (upl[k] < total && P.stop > 8u * (upl[k] - std::min<uint64_t>(upl[k], shift))) { /* it ran into bytes that had not arrived: once more, with more of them */
            rc = ensure_uploaded(up + stage_bytes);
            if (rc) return rc;
            redo = k;
            break;
          }
          if (P.status == MK_INFL_MISSED && P.end != MK_GUN_NONE && P.stop > P.end) {
            while (found < NB && 8u * found * G.batch * S <= P.stop) { rc = find_batch(found++); if (rc) return rc; } /* every candidate in front of stop is known */
            size_t a = gi + 1, b = a;
            while (b < starts.size() && starts[b] < P.stop) b++;
            res.repairs += b - a;
            starts.erase(starts.begin() + a, starts.begin() + b);
            kinds.erase(kinds.begin() + a, kinds.begin() + b);
            const bool known = a < starts.size() && starts[a] == P.stop;
            if (!known) { starts.insert(starts.begin() + a, P.stop); kinds.insert(kinds.begin() + a, 0); }
            uint32_t d = k + 1;
            while (d < T.size() && T[d].start < P.stop) d++;
            drop(k + 1, d);
            mk_gun_piece &Q = T[k]; /* (P may have moved) */
            Q.status = MK_INFL_OK;
            Q.end = Q.stop;
            if (!known && Q.stop < bit_end) { /* the resumed piece is this batch's */
              rc = know_next(a);
              if (rc) return rc;
              mk_gun_piece N;
              memset(&N, 0, sizeof N);
              N.start = Q.stop;
              N.end = a + 1 < starts.size() ? starts[a + 1] : MK_GUN_NONE;
              T.insert(T.begin() + k + 1, N);
              decoded.insert(decoded.begin() + k + 1, 0);
              merges.insert(merges.begin() + k + 1, 0);
              upl.insert(upl.begin() + k + 1, 0);
            }
            continue;
          }
          if (P.status == MK_INFL_CAPACITY && P.end != MK_GUN_NONE && merges[k] < MK_GUNZIP_REPAIR_MERGES) {
            rc = know_next(gi + 1);
            if (rc) return rc;
            starts.erase(starts.begin() + gi + 1);
            kinds.erase(kinds.begin() + gi + 1);
            res.repairs++;
            if (k + 1 < T.size()) drop(k + 1, k + 2);
            mk_gun_piece &Q = T[k];
            Q.end = gi + 1 < starts.size() ? starts[gi + 1] : MK_GUN_NONE;
            merges[k]++;
            redo = k;
            resize = true;
            break;
          }
          stands = true; /* the call's status */
          break;
        }
        if (redo < 0) break; /* every piece is confirmed, or one's status stands */
        mk_gun_piece &P = T[redo];
        if (resize) { /* its symbols at the tail of the buffer */
          const uint64_t covered = (P.end == MK_GUN_NONE ? pay_len : (P.end + 7u) >> 3) - (P.start >> 3);
          const uint64_t cap = (uint64_t)G.ratio * covered;
          if (cap >= ((uint64_t)1 << 31) || nsyms + cap >= ((uint64_t)1 << 32)) {
            (void)hipStreamSynchronize(R.S); (void)hipStreamSynchronize(R.copy);
            res.status = MK_INFL_CAPACITY; res.bad_piece = (int64_t)(idx + redo);
            return MK_OK;
          }
          P.cap = (uint32_t)cap;
          P.sym_off = nsyms;
          nsyms += (cap + 7u) & ~(uint64_t)7u;
          if (nsyms > R.syms_cap) { /* grow with the content kept: the other pieces' symbols stay where they are */
            const uint64_t c = nsyms + nsyms / 8 + 256;
            uint16_t *nw = nullptr;
            MK_GUN_HIP(mk_dev_alloc(&nw, (size_t)c * sizeof(uint16_t)));
            const hipError_t cr = hipMemcpyAsync(nw, R.d_syms, (size_t)P.sym_off * sizeof(uint16_t), hipMemcpyDeviceToDevice, R.S);
            const hipError_t sr = hipStreamSynchronize(R.S);
            (void)hipFree(R.d_syms);
            R.d_syms = nw;
            R.syms_cap = c;
            MK_GUN_HIP(cr);
            MK_GUN_HIP(sr);
          }
        }
        P.status = 0; P.len = 0; P.stop = 0;
        rc = ensure_uploaded(P.end == MK_GUN_NONE ? total : shift + (P.end >> 3) + 4096u);
        if (rc) return rc;
        upl[redo] = up;
        decoded[redo] = 1;
        R.h_pieces[0] = P;
        MK_GUN_HIP(hipMemcpyAsync(R.d_pieces, R.h_pieces, sizeof(mk_gun_piece), hipMemcpyHostToDevice, R.S));
        MK_GUN_HIP(hipEventRecord(R.ev_t[2], R.S));
        hipLaunchKernelGGL(mk_gun_decode_kernel<false>, dim3(1), dim3(64 * MK_INFL_WAVES), 0, R.S, (const uint8_t *)R.d_comp, shift, pay_len, R.d_pieces, 1u, R.d_syms, R.d_mems);
        MK_GUN_HIP(hipGetLastError());
        MK_GUN_HIP(hipEventRecord(R.ev_t[3], R.S));
        MK_GUN_HIP(hipMemcpyAsync(R.h_pieces, R.d_pieces, sizeof(mk_gun_piece), hipMemcpyDeviceToHost, R.S));
        MK_GUN_HIP(hipStreamSynchronize(R.S));
        MK_GUN_HIP(hipEventElapsedTime(&ms, R.ev_t[2], R.ev_t[3]));
        res.decode_ms += ms;
        T[redo] = R.h_pieces[0];
        k = (uint32_t)redo;
      }
      np = (uint32_t)T.size(); /* never more than it was: a resumed piece takes the place of a dropped one */
      memcpy(R.h_pieces, T.data(), (size_t)np * sizeof(mk_gun_piece));
      idx_end = idx + np;
      final = idx_end == starts.size();
    }
    uint64_t ntext = 0;
    uint32_t nrec = 0;
    for (uint32_t k = 0; k < np; k++) {
      mk_gun_piece &P = R.h_pieces[k];
      if (pieces_out) pieces_out->push_back(mk_gunzip_piece{P.start | (P.kind & MK_GUN_K_MEMBER ? MK_GUNZIP_PIECE_MEMBER : 0u), P.len});
      res.npieces++;
      if (P.status) {
        (void)hipStreamSynchronize(R.copy);
        res.status = (int32_t)P.status; res.bad_piece = (int64_t)(idx + k);
        return MK_OK;
      }
      if (P.len > P.cap) { snprintf(R.err, sizeof R.err, "piece %llu reports more symbols than its capacity", (unsigned long long)(idx + k)); return MK_ERR_HIP; }
      if (P.nmem > P.mem_cap) { snprintf(R.err, sizeof R.err, "piece %llu reports more members than it has room for", (unsigned long long)(idx + k)); return MK_ERR_HIP; }
      P.text_off = MK_FQ_CARRY + ntext;
      ntext += P.len;
      P.rec_off = nrec;
      nrec += P.nmem;
    }
    /* chain, resolve, CRC */
    MK_GUN_HIP(mk_grow(&R.d_text, &R.text_cap, mk_fq_buf_bytes(MK_FQ_CARRY + ntext), false));
    MK_GUN_HIP(hipMemcpyAsync(R.d_pieces, R.h_pieces, (size_t)np * sizeof(mk_gun_piece), hipMemcpyHostToDevice, R.S));
    if (nrec) { /* the members that ended in this batch: their ends in its text, their trailers */
      MK_GUN_HIP(mk_grow(&R.d_dense, &R.dense_cap, nrec, false));
      MK_GUN_HIP(mk_grow(&R.h_dense, &R.hdense_cap, nrec, true));
      hipLaunchKernelGGL(mk_gun_members_kernel, dim3(np), dim3(64), 0, R.S, (const mk_gun_piece *)R.d_pieces, (const mk_gun_member *)R.d_mems, R.d_dense);
      MK_GUN_HIP(hipGetLastError());
      MK_GUN_HIP(hipMemcpyAsync(R.h_dense, R.d_dense, (size_t)nrec * sizeof(mk_gun_member), hipMemcpyDeviceToHost, R.S));
      MK_GUN_HIP(hipStreamSynchronize(R.S));
    }
    /* one segment per member range of the batch's text, split where it would exceed 1 GiB; empty members have one, the open
     * range behind the last end has one when it holds text */
    segs.clear();
    {
      uint64_t a = 0;
      for (uint32_t m = 0; m <= nrec; m++) {
        const uint64_t e = m < nrec ? R.h_dense[m].at : ntext;
        if (e < a || e > ntext) { snprintf(R.err, sizeof R.err, "member ends out of order in batch %llu", (unsigned long long)bt); return MK_ERR_HIP; }
        if (m == nrec && e == a) break;
        do {
          const uint64_t n = std::min<uint64_t>(MK_GUN_CRC_SEG, e - a);
          const bool closes = m < nrec && a + n == e;
          segs.push_back(mk_gun_member{closes ? 1u : 0u, closes ? R.h_dense[m].crc32 : 0u, closes ? R.h_dense[m].isize : 0u, (uint32_t)n});
          a += n;
        } while (a < e);
      }
    }
    const uint32_t nseg = (uint32_t)segs.size();
    MK_GUN_HIP(hipMemcpyAsync(R.d_win, R.d_wcarry, MK_GUN_WINDOW, hipMemcpyDeviceToDevice, R.S));
    MK_GUN_HIP(hipEventRecord(R.ev_t[4], R.S));
    hipLaunchKernelGGL(mk_gun_chain_kernel, dim3(1), dim3(1024), 0, R.S, (const mk_gun_piece *)R.d_pieces, np, (const uint16_t *)R.d_syms, R.d_win);
    hipLaunchKernelGGL(mk_gun_resolve_kernel, dim3(64, np), dim3(256), 0, R.S, (const mk_gun_piece *)R.d_pieces, (const uint16_t *)R.d_syms, (const uint8_t *)R.d_win, R.d_text);
    MK_GUN_HIP(hipGetLastError());
    MK_GUN_HIP(hipMemcpyAsync(R.d_wcarry, R.d_win + (uint64_t)np * MK_GUN_WINDOW, MK_GUN_WINDOW, hipMemcpyDeviceToDevice, R.S));
    uint32_t nslices = 0;
    if (nseg) {
      const size_t tab_bytes = mk_gz_table_bytes(nseg);
      MK_GUN_HIP(mk_grow(&R.h_crctab, &R.hcrctab_cap, tab_bytes, true));
      MK_GUN_HIP(mk_grow(&R.d_crctab, &R.crctab_cap, tab_bytes, false));
      mk_infl_blk *tab = (mk_infl_blk *)R.h_crctab;
      uint32_t *slice0s = (uint32_t *)(R.h_crctab + mk_gz_slice0_at(nseg));
      uint64_t at = 0;
      for (uint32_t f = 0; f < nseg; f++) {
        const uint32_t n = segs[f].pad;
        tab[f] = mk_infl_blk{0u, 0u, (uint32_t)(MK_FQ_CARRY + at), n, 0u};
        slice0s[f] = nslices;
        nslices += mk_gz_slices(n);
        at += n;
      }
      slice0s[nseg] = nslices;
      /* the work words: status[nseg] (zeros) | crc[nseg] | slice registers[nslices] */
      MK_GUN_HIP(mk_grow(&R.d_crcwork, &R.crcwork_cap, 2u * (uint64_t)nseg + nslices, false));
      MK_GUN_HIP(mk_grow(&R.h_crc, &R.hcrc_cap, nseg, true));
      MK_GUN_HIP(hipMemcpyAsync(R.d_crctab, R.h_crctab, tab_bytes, hipMemcpyHostToDevice, R.S));
      MK_GUN_HIP(hipMemsetAsync(R.d_crcwork, 0, (size_t)nseg * sizeof(uint32_t), R.S));
      const mk_infl_blk *d_tab = (const mk_infl_blk *)R.d_crctab;
      const uint32_t *d_slice0s = (const uint32_t *)(R.d_crctab + mk_gz_slice0_at(nseg));
      if (nslices) hipLaunchKernelGGL(mk_crc32_files_kernel, dim3((nslices + 3u) / 4u), dim3(256), 0, R.S, (const uint8_t *)R.d_text, d_tab, d_slice0s, nseg, nslices, R.d_crcwork + 2u * (size_t)nseg);
      hipLaunchKernelGGL(mk_crc32_combine_kernel, dim3((nseg + 63u) / 64u), dim3(64), 0, R.S, d_tab, d_slice0s, nseg, (const uint32_t *)(R.d_crcwork + 2u * (size_t)nseg), R.d_crcwork, R.d_crcwork + nseg);
      MK_GUN_HIP(hipGetLastError());
      MK_GUN_HIP(hipMemcpyAsync(R.h_crc, R.d_crcwork + nseg, (size_t)nseg * sizeof(uint32_t), hipMemcpyDeviceToHost, R.S));
    }
    MK_GUN_HIP(hipEventRecord(R.ev_t[5], R.S));
    if (!final) { rc = ensure_uploaded(shift + (bt + 3) * G.batch * S + 4096u); if (rc) return rc; } /* the next batches' bytes travel beside this one's work */
    rc = sink(R.d_text, ntext, final);
    if (rc) { (void)hipStreamSynchronize(R.S); (void)hipStreamSynchronize(R.copy); return rc; }
    MK_GUN_HIP(hipStreamSynchronize(R.S));
    MK_GUN_HIP(hipEventElapsedTime(&ms, R.ev_t[4], R.ev_t[5]));
    res.resolve_ms += ms;
    for (uint32_t f = 0; f < nseg; f++) {
      const uint64_t n = segs[f].pad;
      crc = mk_crc_concat(crc, R.h_crc[f], n);
      crc_len += n;
      if (segs[f].at) { /* the member ends here: its own trailer */
        if (!member_status) member_status = (uint32_t)crc_len != segs[f].isize ? MK_INFL_OUTPUT_LEN : crc != segs[f].crc32 ? MK_INFL_CRC : MK_INFL_OK;
        res.members++;
        crc = 0;
        crc_len = 0;
      }
    }
    res.text_len += ntext;
    idx = idx_end;
  }
  MK_GUN_HIP(hipStreamSynchronize(R.S));
  MK_GUN_HIP(hipStreamSynchronize(R.copy));
  res.members++; /* the last one, whose trailer lies behind the payload */
  if (member_status) res.status = member_status;
  else if ((uint32_t)crc_len != info.isize) res.status = MK_INFL_OUTPUT_LEN;
  else if (crc != info.crc32) res.status = MK_INFL_CRC;
  return MK_OK;
}

} /* namespace */

extern "C" void mk_gunzip_pieces_free(mk_gunzip_pieces *p) {
  if (!p) return;
  free(p->v);
  p->v = nullptr;
  p->n = 0;
}

extern "C" int mk_inflate_stream(mk_inflate *h, const uint8_t *comp, size_t comp_bytes, const mk_gzip_info *info, const mk_gunzip_opts *opts,
                                 uint8_t *text_out, size_t cap, uint64_t *text_len, int32_t *status, mk_gunzip_pieces *pieces) {
  if (!h || !comp || !info || !text_len || !status || (!text_out && cap)) return MK_ERR_ARG;
  *text_len = 0;
  *status = MK_INFL_OK;
  if (pieces) { pieces->v = nullptr; pieces->n = 0; }
  MK_INFL_HIP(h, hipSetDevice(h->device));
  mk_gun_run R;
  R.S = h->stream;
  mk_gun_result res;
  std::vector<mk_gunzip_piece> tab;
  uint64_t done = 0;
  bool fits = true;
  auto read = [&](uint64_t off, uint64_t n, uint8_t *dst) -> int { memcpy(dst, comp + off, n); return MK_OK; };
  auto sink = [&](uint8_t *d_text, uint64_t n, bool) -> int {
    if (done + n > cap) fits = false;
    else if (n && hipMemcpyAsync(text_out + done, d_text + MK_FQ_CARRY, n, hipMemcpyDeviceToHost, R.S) != hipSuccess) return MK_ERR_HIP;
    done += n;
    return MK_OK;
  };
  const int rc = mk_gun_stream(R, comp_bytes, *info, opts, read, sink, &tab, res);
  if (rc) return mk_infl_fail(h, rc, "mk_inflate_stream: %s", R.err[0] ? R.err : "copying the text back failed");
  *text_len = res.text_len;
  *status = res.status;
  h->inflate_ms = res.find_ms + res.decode_ms + res.resolve_ms;
  h->stream_members = res.members;
  h->stream_repairs = res.repairs;
  if (pieces && !tab.empty()) {
    pieces->v = (mk_gunzip_piece *)malloc(tab.size() * sizeof(mk_gunzip_piece));
    if (!pieces->v) return MK_ERR_NOMEM;
    memcpy(pieces->v, tab.data(), tab.size() * sizeof(mk_gunzip_piece));
    pieces->n = tab.size();
  }
  if (!fits && !res.status) return mk_infl_fail(h, MK_ERR_ARG, "mk_inflate_stream: the text has %llu bytes, cap is %llu", (unsigned long long)res.text_len, (unsigned long long)cap);
  return MK_OK;
}

extern "C" int mk_inflate_stream_members(mk_inflate *h, uint64_t *members) {
  if (!h || !members) return MK_ERR_ARG;
  *members = h->stream_members;
  return MK_OK;
}

extern "C" int mk_inflate_stream_repairs(mk_inflate *h, uint64_t *repairs) {
  if (!h || !repairs) return MK_ERR_ARG;
  *repairs = h->stream_repairs;
  return MK_OK;
}

/* both readers' route: occ == false is mk_fastq_frame's rule (-A), occ == true mk_fastq_frame_q's (quality mask qmin), one row a
 * record.  What the second needs from the sink: the file's record count (stats.rows), which decides the first-record exception -- it can only arise in the last slice of the last batch, whose text [t0, e1) is then the
 * whole file: everything in front of it went through the carry, possibly in front of an empty batch. */
static int mk_push_gzip(mk_engine *e, int fd, size_t size, const mk_gunzip_opts *opts, bool occ, int32_t qmin, uint64_t first_ordinal, mk_gunzip_stats *st) {
  if (!e || fd < 0) return MK_ERR_ARG;
  mk_gunzip_stats stats;
  memset(&stats, 0, sizeof stats);
  stats.bad_piece = -1;
  if (st) *st = stats;
  (void)mk_engine_note_gunzip_repairs(e, 0);
  const double t_begin = mk_now_s();
  mk_gzip_info info;
  int rc = mk_gzip_scan_stream(fd, nullptr, size, &info);
  if (rc) return rc;
  if (!info.is_single) { snprintf(mk_bgzf_err, sizeof mk_bgzf_err, "not a single-member gzip file"); return MK_ERR_ARG; }
  void *sp = nullptr;
  int device = 0;
  rc = mk_engine_get_stream(e, &sp, &device);
  if (rc) return rc;
  mk_fq_framer F;
  mk_gun_run R;
  R.S = (hipStream_t)sp;
  hipStream_t S = R.S;
  MK_GUN_HIP(hipSetDevice(device));
  MK_GUN_HIP(F.setup(occ, qmin));
  MK_GUN_HIP(mk_dev_alloc(&R.d_fcarry, (size_t)MK_FQ_CARRY));

  uint32_t carry = 0; /* bytes behind the last complete record, kept in R.d_fcarry between batches */
  bool long_line = false;
  auto read = [&](uint64_t off, uint64_t n, uint8_t *dst) -> int {
    for (uint64_t got = 0; got < n;) {
      const ssize_t r = pread(fd, dst + got, n - got, (off_t)(off + got));
      if (r <= 0) return MK_ERR_IO;
      got += (uint64_t)r;
    }
    return MK_OK;
  };
  mk_fq_handed out{};
  auto push = [&](const uint8_t *d_rows, uint32_t stride, uint32_t nrows) -> int {
    return mk_sketch_push_reads_device(e, d_rows, stride, nrows, first_ordinal + stats.rows + out.rows);
  };
  auto sink = [&](uint8_t *d_text, uint64_t n, bool final_batch) -> int {
    if (n == 0 && !final_batch) return MK_OK;
    const uint64_t text_end = MK_FQ_CARRY + std::min<uint64_t>(n, MK_GUN_SLICE); /* a slice with its carry; its rows are lines of the text, padded */
    MK_GUN_HIP(F.reserve(S, text_end, std::max<uint64_t>(text_end, (uint64_t)8 << 20) + 4096u));
    if (carry) {
      hipLaunchKernelGGL(mk_fq_carry_kernel, dim3((carry + 255u) / 256u), dim3(256), 0, S, (const uint8_t *)R.d_fcarry, 0u, d_text, MK_FQ_CARRY - carry, carry);
      MK_GUN_HIP(hipGetLastError());
    }
    uint64_t off = 0;
    do {
      const uint32_t sl = (uint32_t)std::min<uint64_t>(MK_GUN_SLICE, n - off);
      const int final = final_batch && off + sl == n;
      uint8_t *base = d_text + off;
      const uint32_t t0 = MK_FQ_CARRY - carry, e1 = MK_FQ_CARRY + sl;
      MK_GUN_HIP(F.count(S, base, t0, e1, final, nullptr, 0));
      mk_fq_chunk q;
      MK_GUN_HIP(F.result(stats.rows, &q));
      float ms = 0.f, rows_ms = 0.f; /* frame_ms is the count phase alone on this route */
      MK_GUN_HIP(F.times(&ms, &rows_ms));
      stats.frame_ms += ms;
      if (q.long_line) { long_line = true; return MK_ERR_FORMAT; }
      MK_GUN_HIP(F.rows(S, q, push, &out));
      if (out.push_rc) { snprintf(R.err, sizeof R.err, "%s", mk_last_error(e)); return out.push_rc; }
      stats.rows += out.rows;
      carry = out.carry;
      off += sl;
      if (off >= n && carry) { /* behind the batch's last slice: what is left waits for the next batch's text */
        hipLaunchKernelGGL(mk_fq_carry_kernel, dim3((carry + 255u) / 256u), dim3(256), 0, S, (const uint8_t *)base, t0 + q.r.consumed, R.d_fcarry, 0u, carry);
        MK_GUN_HIP(hipGetLastError());
      }
    } while (off < n);
    return MK_OK;
  };
  mk_gun_result res;
  rc = mk_gun_stream(R, size, info, opts, read, sink, nullptr, res);
  (void)hipStreamSynchronize(S);
  stats.pieces = res.npieces; stats.batches = res.nbatches; stats.comp_bytes = size; stats.text_bytes = res.text_len;
  stats.find_ms = res.find_ms; stats.decode_ms = res.decode_ms; stats.resolve_ms = res.resolve_ms; stats.t_read_s = res.t_read_s;
  stats.bad_piece = res.bad_piece; stats.bad_status = res.status; stats.members = (uint32_t)std::min<uint64_t>(res.members, 0xffffffffu);
  stats.t_total_s = mk_now_s() - t_begin;
  (void)mk_engine_note_gunzip_repairs(e, res.repairs);
  if (st) *st = stats;
  if (rc == MK_ERR_FORMAT && long_line) { snprintf(mk_bgzf_err, sizeof mk_bgzf_err, "a FASTQ line of 4095 characters or more"); return rc; }
  if (rc) { snprintf(mk_bgzf_err, sizeof mk_bgzf_err, "%s", R.err); return rc; }
  if (res.status) {
    snprintf(mk_bgzf_err, sizeof mk_bgzf_err, "gzip stream, piece %lld: %s", (long long)res.bad_piece, mk_gunzip_status_text(res.status));
    return MK_ERR_FORMAT;
  }
  return MK_OK;
}

/* The long sink: the same stream decode, every batch's text to mk_sketch_push_fastq_long_device.  The engine copies
 * the text into its own buffer on R.S, which is its stream, so R.d_text is free for the next batch's resolve; the open record waits
 * in the engine.  No framer, no carry of this route's, no slices: a batch holds less than 2^31 bytes of text. */
static int mk_push_gzip_long(mk_engine *e, int fd, size_t size, const mk_gunzip_opts *opts, int final, mk_gunzip_stats *st, bool q, int32_t qmin) {
  if (!e || fd < 0) return MK_ERR_ARG;
  auto long_push = [&](const uint8_t *d, uint64_t n, int fin) -> int { /* q: fastq2co's rule with its mask */
    return q ? mk_sketch_push_fastq_long_q_device(e, d, n, fin, qmin) : mk_sketch_push_fastq_long_device(e, d, n, fin);
  };
  mk_gunzip_stats stats;
  memset(&stats, 0, sizeof stats);
  stats.bad_piece = -1;
  if (st) *st = stats;
  (void)mk_engine_note_gunzip_repairs(e, 0);
  const double t_begin = mk_now_s();
  mk_gzip_info info;
  int rc = mk_gzip_scan_stream(fd, nullptr, size, &info);
  if (rc) return rc;
  if (!info.is_single) { snprintf(mk_bgzf_err, sizeof mk_bgzf_err, "not a single-member gzip file"); return MK_ERR_ARG; }
  void *sp = nullptr;
  int device = 0;
  rc = mk_engine_get_stream(e, &sp, &device);
  if (rc) return rc;
  mk_gun_run R;
  R.S = (hipStream_t)sp;
  MK_GUN_HIP(hipSetDevice(device));
  double frame0 = 0;
  if ((rc = mk_sketch_fastq_long_frame_ms(e, &frame0))) { snprintf(mk_bgzf_err, sizeof mk_bgzf_err, "%s", mk_last_error(e)); return rc; }
  auto read = [&](uint64_t off, uint64_t n, uint8_t *dst) -> int {
    for (uint64_t got = 0; got < n;) {
      const ssize_t r = pread(fd, dst + got, n - got, (off_t)(off + got));
      if (r <= 0) return MK_ERR_IO;
      got += (uint64_t)r;
    }
    return MK_OK;
  };
  bool closed = false;
  auto sink = [&](uint8_t *d_text, uint64_t n, bool final_batch) -> int {
    const int fin = final && final_batch;
    if (n == 0 && !fin) return MK_OK;
    const int prc = long_push(d_text + MK_FQ_CARRY, n, fin);
    if (prc) snprintf(R.err, sizeof R.err, "%s", mk_last_error(e));
    else if (fin) closed = true;
    return prc;
  };
  mk_gun_result res;
  rc = mk_gun_stream(R, size, info, opts, read, sink, nullptr, res);
  if (!rc && !res.status && final && !closed) { /* (no batch called itself the last one: the stream had no piece to give) */
    rc = long_push(nullptr, 0, 1);
    if (rc) snprintf(R.err, sizeof R.err, "%s", mk_last_error(e));
  }
  (void)hipStreamSynchronize(R.S);
  double frame1 = frame0;
  (void)mk_sketch_fastq_long_frame_ms(e, &frame1);
  stats.frame_ms = frame1 - frame0;
  stats.pieces = res.npieces; stats.batches = res.nbatches; stats.comp_bytes = size; stats.text_bytes = res.text_len;
  stats.find_ms = res.find_ms; stats.decode_ms = res.decode_ms; stats.resolve_ms = res.resolve_ms; stats.t_read_s = res.t_read_s;
  stats.bad_piece = res.bad_piece; stats.bad_status = res.status; stats.members = (uint32_t)std::min<uint64_t>(res.members, 0xffffffffu);
  stats.t_total_s = mk_now_s() - t_begin;
  (void)mk_engine_note_gunzip_repairs(e, res.repairs);
  if (st) *st = stats;
  if (rc) { snprintf(mk_bgzf_err, sizeof mk_bgzf_err, "%s", R.err); return rc; }
  if (res.status) {
    snprintf(mk_bgzf_err, sizeof mk_bgzf_err, "gzip stream, piece %lld: %s", (long long)res.bad_piece, mk_gunzip_status_text(res.status));
    return MK_ERR_FORMAT;
  }
  return MK_OK;
}

extern "C" int mk_sketch_push_gzip_long(mk_engine *e, int fd, size_t size, const mk_gunzip_opts *opts, int final, mk_gunzip_stats *st) {
  return mk_push_gzip_long(e, fd, size, opts, final, st, false, 0);
}

extern "C" int mk_sketch_push_gzip_long_q(mk_engine *e, int fd, size_t size, const mk_gunzip_opts *opts, int32_t qmin, int final, mk_gunzip_stats *st) {
  return mk_push_gzip_long(e, fd, size, opts, final, st, true, qmin);
}

extern "C" int mk_sketch_push_gzip(mk_engine *e, int fd, size_t size, const mk_gunzip_opts *opts, uint64_t first_ordinal, mk_gunzip_stats *st) {
  return mk_push_gzip(e, fd, size, opts, false, 0, first_ordinal, st);
}

extern "C" int mk_sketch_push_gzip_q(mk_engine *e, int fd, size_t size, const mk_gunzip_opts *opts, int32_t qmin, uint64_t first_ordinal, mk_gunzip_stats *st) {
  return mk_push_gzip(e, fd, size, opts, true, qmin, first_ordinal, st);
}
