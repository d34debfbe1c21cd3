/* mk_gzip.c -- the header and trailer of a plain gzip file (RFC 1952), as genome archives write their `.fna.gz`: ONE member, any
 * of the optional header fields.  The walk answers "where does the deflate stream lie, and what do the last eight bytes promise
 * about its text?" for a file that has this shape:
 *   1f 8b 08 | FLG (reserved bits 5-7 zero) | MTIME XFL OS | [FEXTRA: XLEN + bytes] [FNAME: ..0] [FCOMMENT: ..0] [FHCRC: 2 bytes,
 *   not verified] | payload | CRC32 ISIZE
 * with 1 <= ISIZE <= MK_BATCH_FILE_MAX.  Anything else -- a header that runs past the file, reserved bits, another method, an
 * empty file, ISIZE 0 -- is "not for the device": is_single = 0 with MK_OK, and the caller keeps the `zcat -fc` route.  A
 * concatenation of members passes (its last eight bytes are a trailer too): only the decode can tell, and says
 * MK_INFL_TRAILING.  Host code only. */
#include "metakssd_hip.h"
#include "mk_host_internal.h"

#include <string.h>
#include <sys/mman.h>

static inline uint32_t mk_gz_le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
static inline uint32_t mk_gz_le32(const uint8_t *p) { return mk_gz_le16(p) | mk_gz_le16(p + 2) << 16; }

/* the first byte behind the header, 0 = none inside [0, size) */
static size_t mk_gzip_header_end(const uint8_t *p, size_t size) {
  if (size < 10u || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || (p[3] & 0xe0u)) return 0;
  const uint32_t flg = p[3];
  size_t at = 10;
  if (flg & 4u) { /* FEXTRA */
    if (size - at < 2u) return 0;
    const size_t xlen = mk_gz_le16(p + at);
    at += 2;
    if (size - at < xlen) return 0;
    at += xlen;
  }
  for (uint32_t bit = 8u; bit <= 16u; bit <<= 1) { /* FNAME, FCOMMENT: zero-terminated */
    if (!(flg & bit)) continue;
    const uint8_t *z = memchr(p + at, 0, size - at);
    if (!z) return 0;
    at = (size_t)(z - p) + 1u;
  }
  if (flg & 2u) { /* FHCRC */
    if (size - at < 2u) return 0;
    at += 2;
  }
  return at;
}

/* stream != 0: mk_gzip_scan_stream's rule -- ISIZE is the text length mod 2^32 and says nothing about the size, and the payload
 * may be of any length */
static int mk_gzip_scan_any(int fd, const uint8_t *mem, size_t size, mk_gzip_info *out, int stream) {
  if (!out || (!mem && fd < 0)) return MK_ERR_ARG;
  memset(out, 0, sizeof *out);
  if (size < 10u + 1u + 8u) return MK_OK; /* the fixed header, one byte of deflate, the trailer */
  const uint8_t *p = mem;
  if (!p) { /* only the header and the trailer are touched */
    p = mmap(NULL, size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (p == MAP_FAILED) return MK_ERR_IO;
  }
  const size_t pay = mk_gzip_header_end(p, size);
  if (pay && size - pay >= 1u + 8u && (stream || size - pay - 8u < ((uint64_t)1 << 31))) {
    const uint32_t isize = mk_gz_le32(p + size - 4);
    if (stream || (isize >= 1u && isize <= MK_BATCH_FILE_MAX)) {
      out->pay_off = pay;
      out->pay_len = size - pay - 8u;
      out->crc32 = mk_gz_le32(p + size - 8);
      out->isize = isize;
      out->is_single = 1;
    }
  }
  if (!mem) munmap((void *)p, size);
  return MK_OK;
}

int mk_gzip_scan(int fd, const uint8_t *mem, size_t size, mk_gzip_info *out) { return mk_gzip_scan_any(fd, mem, size, out, 0); }

int mk_gzip_scan_stream(int fd, const uint8_t *mem, size_t size, mk_gzip_info *out) { return mk_gzip_scan_any(fd, mem, size, out, 1); }
