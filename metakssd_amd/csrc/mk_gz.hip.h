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
