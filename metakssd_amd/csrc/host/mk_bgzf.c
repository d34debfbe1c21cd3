/* mk_bgzf.c -- recognise and walk a BGZF file (what `bgzip` writes): a chain of independent gzip members of at most 64 KiB of
 * text each, every member with its compressed size in a 'B','C' extra subfield and its uncompressed size in its trailer.  The
 * walk answers one question for the whole file -- "is every byte of it part of such a chain?" -- and, if so, leaves a table with
 * one entry per member.  Every ISIZE is known here, so where a member's text goes in the output is a host prefix sum.
 * Anything else (a plain gzip member anywhere, trailing bytes, a member cut off by the end of the file) is "not BGZF": the caller
 * keeps the `zcat -fc` route (iseq2comem.c:666-669) for the whole file.  Host code only. */
#include "metakssd_hip.h"
#include "mk_host_internal.h"

#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>

static inline uint32_t mk_le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
static inline uint32_t mk_le32(const uint8_t *p) { return mk_le16(p) | mk_le16(p + 2) << 16; }

/* the member at p (avail bytes up to the end of the file): 0 = not a BGZF member */
static int mk_bgzf_member(const uint8_t *p, size_t avail, mk_bgzf_block *b) {
  if (avail < 12u + 6u + 8u) return 0;
  if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) return 0; /* gzip, deflate, FLG == FEXTRA exactly */
  const uint32_t xlen = mk_le16(p + 10);
  if (12u + (size_t)xlen + 8u > avail) return 0;
  int have_bc = 0;
  uint32_t bsize = 0, at = 0;
  while (at + 4u <= xlen) { /* subfields: SI1 SI2 SLEN data */
    const uint8_t *f = p + 12 + at;
    const uint32_t slen = mk_le16(f + 2);
    if (at + 4u + slen > xlen) return 0;
    if (f[0] == 'B' && f[1] == 'C') {
      if (slen != 2 || have_bc) return 0;
      have_bc = 1;
      bsize = mk_le16(f + 4);
    }
    at += 4u + slen;
  }
  if (at != xlen || !have_bc) return 0;
  const size_t total = (size_t)bsize + 1u; /* BSIZE = member size - 1 */
  if (total < 12u + (size_t)xlen + 8u || total > avail) return 0; /* BSIZE keeps the member inside the file */
  const uint32_t isize = mk_le32(p + total - 4);
  if (isize > 65536u) return 0;
  b->in_len = (uint32_t)total;
  b->pay_off = 12u + xlen;
  b->pay_len = (uint32_t)total - 12u - xlen - 8u;
  b->crc32 = mk_le32(p + total - 8);
  b->isize = isize;
  b->reserved = 0;
  return 1;
}

int mk_bgzf_scan(int fd, const uint8_t *mem, size_t size, mk_bgzf_block **blocks, uint64_t *nblocks, uint64_t *total_out, int *is_bgzf) {
  if (!blocks || !nblocks || !is_bgzf || (!mem && fd < 0)) return MK_ERR_ARG;
  *blocks = NULL; *nblocks = 0; *is_bgzf = 0;
  if (total_out) *total_out = 0;
  if (size == 0) return MK_OK;
  const uint8_t *p = mem;
  if (!p) { /* only the headers and trailers are touched: two pages a member */
    p = mmap(NULL, size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (p == MAP_FAILED) return MK_ERR_IO;
  }
  int rc = MK_OK;
  uint64_t n = 0, cap = 0, out = 0;
  size_t at = 0;
  mk_bgzf_block *t = NULL;
  while (at < size) {
    mk_bgzf_block b;
    if (!mk_bgzf_member(p + at, size - at, &b)) break;
    if (n == cap) {
      cap = cap ? cap * 2 : 1024;
      mk_bgzf_block *t2 = realloc(t, cap * sizeof *t);
      if (!t2) { rc = MK_ERR_NOMEM; break; }
      t = t2;
    }
    b.in_off = at;
    b.out_off = out;
    t[n++] = b;
    out += b.isize;
    at += b.in_len;
  }
  if (!mem) munmap((void *)p, size);
  if (rc != MK_OK || at != size || n == 0) { free(t); return rc; }
  *blocks = t; *nblocks = n; *is_bgzf = 1;
  if (total_out) *total_out = out;
  return MK_OK;
}

void mk_bgzf_free(mk_bgzf_block *blocks) { free(blocks); }

const char *mk_inflate_status_text(int status) {
  switch (status) {
    case MK_INFL_OK: return "ok";
    case MK_INFL_BAD_BLOCK: return "bad deflate block type";
    case MK_INFL_BAD_LENGTHS: return "bad code lengths";
    case MK_INFL_BAD_CODE: return "over-subscribed or incomplete code";
    case MK_INFL_BAD_DISTANCE: return "distance beyond the start of the block's output";
    case MK_INFL_INPUT: return "compressed data exhausted";
    case MK_INFL_OUTPUT_LEN: return "output length not equal to ISIZE";
    case MK_INFL_CRC: return "CRC mismatch";
    case MK_INFL_TRAILING: return "more members behind the first";
    case MK_INFL_MISSED: return "a piece start that is no block start";
    case MK_INFL_CAPACITY: return "a piece's text exceeds its capacity";
    default: return "unknown status";
  }
}

const char *mk_gunzip_status_text(int status) {
  if (status == MK_INFL_BAD_MEMBER) return "no gzip member behind a member's trailer";
  return mk_inflate_status_text(status);
}
