/* mk_gz.hip.h -- what mk_inflate.hip offers the engine (mk_sketch_batch_begin_gz): the member table the inflate kernels read and
 * one call that queues inflate + CRC for a set of plain gzip members on any stream.  Not part of the C ABI. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "metakssd_hip.h"

struct mk_infl_blk { uint32_t pay_off, pay_len, out_off, isize, crc; };

/* slices of MK_CRC_SLICE bytes a text of isize bytes gives the CRC kernel (an empty text has none) */
static inline uint32_t mk_gz_slices(uint32_t isize) { return (isize + MK_CRC_SLICE - 1u) / MK_CRC_SLICE; }
/* the table as it lies on the device: n entries, then (16-byte aligned) the first slice of every member and the total */
static inline size_t mk_gz_slice0_at(uint32_t n) { return ((size_t)n * sizeof(mk_infl_blk) + 15u) & ~(size_t)15u; }
static inline size_t mk_gz_table_bytes(uint32_t n) { return mk_gz_slice0_at(n) + (((size_t)n + 1u) * 4u + 15u & ~(size_t)15u); }
/* the device scratch, in words: status[n] | consumed[n] | pos[n] | crc[n] | slice CRCs[nslices] */
static inline size_t mk_gz_work_words(uint32_t n, uint32_t nslices) { return 4u * (size_t)n + nslices; }

/* Queues on s: every member inflated to its out_off in d_text (no in-wave CRC), the CRC32 of every text by slices, the combine.
 * d_comp: the payloads (offsets of the table are relative to it; 16-byte aligned, 16 bytes of slack behind the last payload),
 * d_tab: mk_gz_table_bytes(n) as laid out above.  When the stream gets there work[0..n) holds the MK_INFL_* statuses. */
hipError_t mk_gz_launch(hipStream_t s, const uint8_t *d_comp, const void *d_tab, uint32_t n, uint32_t nslices, uint8_t *d_text, uint32_t *d_work);

/* ---- the same texts by MANY wavefronts per file (mk_gunzip_batch.hip.h) -----------------------------------------
 * Every payload is cut into spans of S compressed bytes; the spans of a batch are numbered file after file, and every span has a
 * slot in the tables below whether a piece starts in it or not. */
#define MK_GB_SPAN_DEFAULT MK_GUNZIP_BATCH_SPAN_DEFAULT /* S of this route when mk_gunzip_opts.span_bytes is 0 */
#define MK_GB_SYMS_MAX MK_GUNZIP_BATCH_SYMS_MAX         /* 16-bit symbols a batch may need room for: 4 GiB */
#define MK_GB_SPANS_MAX MK_GUNZIP_BATCH_SPANS_MAX       /* spans of a batch: a table slot and a 32 KiB window each (2 GiB), the resolve grid's second dimension */

struct mk_gb_file { /* per file, beside its mk_infl_blk */
  uint64_t sym_base; /* where its symbols start, in units of R symbols: the prefix sum of pay_len + nspans */
  uint32_t span0, nspans; /* its slots */
};
struct mk_gb_geom { uint32_t S, R; };
/* S and R from the options (span_bytes 0: MK_GB_SPAN_DEFAULT, ratio 0: 16; clamped as mk_inflate_stream clamps them).  false: flags set */
bool mk_gb_geometry(const mk_gunzip_opts *o, mk_gb_geom *g);
static inline uint32_t mk_gb_spans(uint64_t pay_len, uint32_t S) { return pay_len ? (uint32_t)((pay_len + S - 1u) / S) : 1u; }
/* ftab[0, n) from the payload lengths of tab; *nspans the slots and *nsyms the symbols the batch needs.  false: more than
 * MK_GB_SPANS_MAX or MK_GB_SYMS_MAX (the counts are still what they are) */
static inline bool mk_gb_plan(const mk_infl_blk *tab, uint32_t n, mk_gb_geom g, mk_gb_file *ftab, uint64_t *nspans, uint64_t *nsyms) {
  uint64_t units = 0, spans = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t ns = mk_gb_spans(tab[i].pay_len, g.S);
    if (ftab) ftab[i] = mk_gb_file{units, (uint32_t)spans, ns};
    spans += ns;
    units += (uint64_t)tab[i].pay_len + ns;
  }
  *nspans = spans;
  *nsyms = units * g.R;
  return spans <= MK_GB_SPANS_MAX && units * g.R <= MK_GB_SYMS_MAX;
}
/* device bytes: the span table (candidates, pieces, links), the windows (one in front of all, one per slot), the symbols */
size_t mk_gb_scratch_bytes(uint64_t nspans);
static inline size_t mk_gb_win_bytes(uint64_t nspans) { return (size_t)(nspans + 1u) * 32768u; }
static inline size_t mk_gb_sym_bytes(uint64_t nsyms) { return (size_t)nsyms * 2u + 16u; }
/* the work words: status[n] | consumed[n] | pos[n] | crc[n] | pieces[n] | slice CRCs[nslices] -- mk_gz_launch's, and the piece counts */
static inline size_t mk_gb_work_words(uint32_t n, uint32_t nslices) { return 5u * (size_t)n + nslices; }
/* Queues on s, without a wait on the host: finder, piece table, decode, window chain, resolve, CRC by slices, combine.  d_tab as for
 * mk_gz_launch, d_ftab what mk_gb_plan made of it.  When the stream gets there work[0, n) holds the MK_INFL_* statuses, d_text every
 * text whose pieces could be resolved, work[4n, 5n) every file's pieces. */
hipError_t mk_gb_launch(hipStream_t s, const uint8_t *d_comp, const void *d_tab, const mk_gb_file *d_ftab, uint32_t n, uint32_t nslices, uint32_t nspans,
                        mk_gb_geom g, void *d_scratch, uint16_t *d_syms, uint8_t *d_win, uint8_t *d_text, uint32_t *d_work);
