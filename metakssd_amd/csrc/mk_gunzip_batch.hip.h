/* mk_gunzip_batch.hip.h -- a BATCH of single-member gzip files, each inflated by many wavefronts (part of mk_inflate.hip, which
 * includes it behind mk_gunzip.hip.h; gfx950, wave64, hand-written).  mk_gunzip.hip.h's two-pass decode, per file,
 * as ONE launch sequence without a wait on the host: what the host did there between the kernels of one stream -- reading the
 * candidates, making the piece table, the prefix sums over the lengths -- is done by kernels here, and every wave looks up the
 * file it works for in a table (mk_infl_blk: where the payload lies, ISIZE, the text's place; mk_gb_file: the file's spans).
 *
 * Spans are numbered through the batch, file after file; slot i of cand[], pieces[] and link[] belongs to span i.
 *   mk_gb_find_kernel     one wave per slot.  Span 0 of a file has no candidate (its piece starts at bit 0); every other span gets
 *                         mk_gun_find_span's answer for the bits [8cS, min(8(c + 1)S, 8 * pay_len)) of ITS FILE's payload.
 *   mk_gb_table_kernel    one thread per slot: span 0 of a file and every span with a candidate start a piece, which ends at the
 *                         next candidate of the same file (MK_GUN_NONE for the file's last); cap = R * (whole bytes covered);
 *                         symbols at R * (sym_base + start / 8 + c) -- compressed offsets alone, and two pieces, which share at
 *                         most the byte the later one starts in, are at least the earlier one's cap apart.  Other slots are empty.
 *   mk_gb_decode_kernel   one wave per slot with a piece: mk_gun_decode_piece<false> with the file's comp, shift and pay_len.
 *   mk_gb_chain_kernel    one WORKGROUP per file, its pieces in order: W(c) from W(c - 1) and piece c's symbols (W in front of a
 *                         file is the zero window 0), text_off = out_off + the lengths so far.  It stops at the first piece with a
 *                         status, or where the lengths would pass ISIZE (MK_INFL_OUTPUT_LEN); pieces from there on are not linked
 *                         and so not resolved.  Leaves the file's status, bytes consumed, text length and piece count in work[].
 *   mk_gb_resolve_kernel  every linked piece at once: text[text_off + i] = sym < 0x8000 ? sym : W(c - 1)[sym & 0x7fff]
 * then mk_crc32_files_kernel and mk_crc32_combine_kernel as in mk_gz_launch, which fold MK_INFL_CRC into a status that is still OK.
 * Status of a file, in order of precedence: the first piece in stream order that has one; MK_INFL_OUTPUT_LEN; MK_INFL_CRC.
 *
 * Safety.  Loads of finder and decode: the file's payload through mk_bits_t<true>, which reads zeros behind the payload's end, so a
 * status depends on the file alone; the finder's four aligned words reach at most 16 bytes behind the payload, into its trailer
 * and the next file or the buffer's slack (such bits never decide: a candidate's fixed header must lie below 8 * pay_len and the
 * whole-wave test reads through mk_bits_t<true>).  Stores: cand[], pieces[], link[] one entry per slot, index tested against the
 * slot count; a piece's symbols inside its cap, tested before every store, and cap + sym_off stays inside the file's
 * R * (pay_len + nspans) symbols; window i + 1 by slot i's piece; text inside [out_off, out_off + ISIZE) because the chain links
 * a piece only while the lengths stay within ISIZE and a length is never above cap; work[] by file index.  Every decode loop
 * consumes input bits or produces symbols (mk_gunzip.hip.h); the table kernel's look-ahead and the chain's walk are bounded by the
 * file's spans.  Damage is a status, never a fault.  MK_POISON: every slot of cand[], pieces[] and link[] is written before it is
 * read, symbols and windows are read only where a piece wrote them.  Plain C++ and vector stores only. */

namespace {

struct mk_gb_link { uint32_t wprev, live; }; /* left by the chain: the window piece's markers index, whether it is resolved */

static_assert(sizeof(mk_gun_piece) % 8u == 0, "the span table's parts are 8-byte aligned");

/* the file slot `slot` belongs to: the last one whose first slot is <= slot (every file has at least one) */
__device__ __forceinline__ uint32_t mk_gb_file_of(const mk_gb_file *__restrict__ ftab, uint32_t nfiles, uint32_t slot) {
  uint32_t lo = 0, hi = nfiles;
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (ftab[mid].span0 <= slot) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(64 * MK_INFL_WAVES) mk_gb_find_kernel(const uint8_t *__restrict__ comp, const mk_infl_blk *__restrict__ blks,
                                                                         const mk_gb_file *__restrict__ ftab, uint32_t nfiles, uint32_t S, uint32_t nslots,
                                                                         uint64_t *cand) {
  __shared__ mk_infl_lds lds_all[MK_INFL_WAVES];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x * MK_INFL_WAVES + wave;
  if (i >= nslots) return;
  const uint32_t f = mk_uni(mk_gb_file_of(ftab, nfiles, i));
  const uint64_t c = i - mk_uni(ftab[f].span0);
  uint64_t found = MK_GUN_NONE;
  if (c) { /* c < nspans: the span starts inside the payload */
    const uint32_t pay_off = mk_uni(blks[f].pay_off), shift = pay_off & 15u;
    const uint64_t pay_len = mk_uni(blks[f].pay_len), nbits = 8u * pay_len;
    const uint64_t lo = 8u * c * S, hi = 8u * (c + 1u) * S < nbits ? 8u * (c + 1u) * S : nbits;
    found = mk_gun_find_span<false>(comp + (pay_off - shift), shift, pay_len, lo, hi, lds_all[wave], lane);
  }
  if (lane == 0u) cand[i] = found;
}

__global__ void __launch_bounds__(256) mk_gb_table_kernel(const mk_infl_blk *__restrict__ blks, const mk_gb_file *__restrict__ ftab, uint32_t nfiles, uint32_t R,
                                                          uint32_t nslots, const uint64_t *__restrict__ cand, mk_gun_piece *pieces, mk_gb_link *link) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= nslots) return;
  const uint32_t f = mk_gb_file_of(ftab, nfiles, i);
  const mk_gb_file F = ftab[f];
  const uint32_t c = i - F.span0;
  mk_gun_piece P;
  memset(&P, 0, sizeof P);
  P.start = c ? cand[i] : 0u;
  P.end = MK_GUN_NONE;
  if (P.start != MK_GUN_NONE) {
    for (uint32_t j = i + 1u; j < F.span0 + F.nspans; j++)
      if (cand[j] != MK_GUN_NONE) { P.end = cand[j]; break; }
    const uint64_t pay_len = blks[f].pay_len;
    const uint64_t covered = (P.end == MK_GUN_NONE ? pay_len : (P.end + 7u) >> 3) - (P.start >> 3);
    P.cap = (uint32_t)((uint64_t)R * covered); /* (below 2^31: the host held R * (pay_len + nspans) against MK_GB_SYMS_MAX) */
    P.first = c == 0u;
    P.sym_off = (uint64_t)R * (F.sym_base + (P.start >> 3) + c);
  }
  pieces[i] = P;
  link[i] = mk_gb_link{0u, 0u};
}

__global__ void __launch_bounds__(64 * MK_INFL_WAVES) mk_gb_decode_kernel(const uint8_t *__restrict__ comp, const mk_infl_blk *__restrict__ blks,
                                                                           const mk_gb_file *__restrict__ ftab, uint32_t nfiles, mk_gun_piece *pieces, uint32_t nslots,
                                                                           uint16_t *syms) {
  __shared__ mk_infl_lds lds_all[MK_INFL_WAVES];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t k = blockIdx.x * MK_INFL_WAVES + wave;
  if (k >= nslots) return;
  if (mk_uni64(pieces[k].start) == MK_GUN_NONE) return; /* no piece starts in this span */
  const uint32_t f = mk_uni(mk_gb_file_of(ftab, nfiles, k));
  const uint32_t pay_off = mk_uni(blks[f].pay_off), shift = pay_off & 15u;
  mk_gun_decode_piece<false>(comp + (pay_off - shift), shift, (uint64_t)mk_uni(blks[f].pay_len), pieces, k, syms, nullptr, lds_all[wave], lane);
}

/* blockIdx.x: the file.  win: window 0 is zeros, window i + 1 becomes W(the piece of slot i).  Every thread loads the same table
 * entries, so the walk is the same in all of them */
__global__ void __launch_bounds__(1024) mk_gb_chain_kernel(const mk_infl_blk *__restrict__ blks, const mk_gb_file *__restrict__ ftab, uint32_t nfiles,
                                                           mk_gun_piece *pieces, mk_gb_link *link, const uint16_t *__restrict__ syms, uint8_t *win, uint32_t *work) {
  const uint32_t f = blockIdx.x, t = threadIdx.x;
  const mk_gb_file F = ftab[f];
  const uint32_t isize = blks[f].isize, out_off = blks[f].out_off, pay_len = blks[f].pay_len;
  uint32_t prev = 0, sum = 0, np = 0, st = MK_INFL_OK;
  uint64_t stop = 0;
  bool open = true; /* no piece so far has ended the walk */
  for (uint32_t c = 0; c < F.nspans; c++) {
    const uint32_t i = F.span0 + c;
    if (pieces[i].start == MK_GUN_NONE) continue;
    np++;
    if (!open) continue;
    const uint32_t n = pieces[i].len;
    stop = pieces[i].stop;
    if (pieces[i].status) { st = pieces[i].status; open = false; continue; }
    if (n > pieces[i].cap) { st = MK_INFL_CAPACITY; open = false; continue; } /* (cannot happen: the decode tests before every store) */
    if (n > isize - sum) { st = MK_INFL_OUTPUT_LEN; open = false; continue; }
    if (t == 0u) {
      pieces[i].text_off = (uint64_t)out_off + sum;
      link[i] = mk_gb_link{prev, 1u};
    }
    const uint16_t *s = syms + pieces[i].sym_off;
    const uint8_t *wp = win + (uint64_t)prev * MK_GUN_WINDOW;
    uint8_t *wn = win + (uint64_t)(i + 1u) * MK_GUN_WINDOW;
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
    prev = i + 1u;
    sum += n;
    __syncthreads(); /* the workgroup's stores to this window are visible to its loads in the next turn */
  }
  if (!st && sum != isize) st = MK_INFL_OUTPUT_LEN;
  if (t == 0u) {
    const uint64_t used = (stop + 7u) >> 3;
    work[f] = st;
    work[nfiles + f] = used < pay_len ? (uint32_t)used : pay_len;
    work[2u * (size_t)nfiles + f] = sum;
    work[4u * (size_t)nfiles + f] = np;
  }
}

/* blockIdx.y: the slot */
__global__ void __launch_bounds__(256) mk_gb_resolve_kernel(const mk_gun_piece *__restrict__ pieces, const mk_gb_link *__restrict__ link,
                                                            const uint16_t *__restrict__ syms, const uint8_t *__restrict__ win, uint8_t *text) {
  const uint32_t c = blockIdx.y;
  if (!link[c].live) return;
  const uint32_t n = pieces[c].len;
  const uint16_t *s = syms + pieces[c].sym_off;
  const uint8_t *w = win + (uint64_t)link[c].wprev * MK_GUN_WINDOW;
  uint8_t *out = text + pieces[c].text_off;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const uint32_t sym = s[i];
    out[i] = (uint8_t)(sym < 0x8000u ? sym : w[sym & 0x7fffu]);
  }
}

/* the span table as it lies in d_scratch: cand[nspans] | pieces[nspans] | link[nspans] */
static inline size_t mk_gb_pieces_at(uint64_t nspans) { return (size_t)nspans * sizeof(uint64_t); }
static inline size_t mk_gb_link_at(uint64_t nspans) { return mk_gb_pieces_at(nspans) + (size_t)nspans * sizeof(mk_gun_piece); }

} /* namespace */

size_t mk_gb_scratch_bytes(uint64_t nspans) { return mk_gb_link_at(nspans) + (size_t)nspans * sizeof(mk_gb_link) + 16u; }

bool mk_gb_geometry(const mk_gunzip_opts *o, mk_gb_geom *g) {
  if (o && o->flags) return false;
  mk_gunzip_opts with = {o && o->span_bytes ? o->span_bytes : MK_GB_SPAN_DEFAULT, o ? o->ratio : 0u, 0u, 0u};
  const mk_gun_geom G = mk_gun_geometry(&with);
  g->S = G.S;
  g->R = G.ratio;
  return true;
}

hipError_t mk_gb_launch(hipStream_t s, const uint8_t *d_comp, const void *d_tab, const mk_gb_file *d_ftab, uint32_t n, uint32_t nslices, uint32_t nspans,
                        mk_gb_geom g, void *d_scratch, uint16_t *d_syms, uint8_t *d_win, uint8_t *d_text, uint32_t *d_work) {
  if (!n) return hipSuccess;
  if (nspans < n || nspans > MK_GB_SPANS_MAX) return hipErrorInvalidValue;
  const mk_infl_blk *blks = (const mk_infl_blk *)d_tab;
  const uint32_t *slice0s = (const uint32_t *)((const uint8_t *)d_tab + mk_gz_slice0_at(n));
  uint64_t *cand = (uint64_t *)d_scratch;
  mk_gun_piece *pieces = (mk_gun_piece *)((uint8_t *)d_scratch + mk_gb_pieces_at(nspans));
  mk_gb_link *link = (mk_gb_link *)((uint8_t *)d_scratch + mk_gb_link_at(nspans));
  uint32_t *slice_crc = d_work + 5u * (size_t)n;
  const uint32_t waves = (nspans + MK_INFL_WAVES - 1u) / MK_INFL_WAVES;
  hipError_t r = hipMemsetAsync(d_win, 0, MK_GUN_WINDOW, s); /* W in front of every file */
  if (r != hipSuccess) return r;
  hipLaunchKernelGGL(mk_gb_find_kernel, dim3(waves), dim3(64 * MK_INFL_WAVES), 0, s, d_comp, blks, d_ftab, n, g.S, nspans, cand);
  hipLaunchKernelGGL(mk_gb_table_kernel, dim3((nspans + 255u) / 256u), dim3(256), 0, s, blks, d_ftab, n, g.R, nspans, (const uint64_t *)cand, pieces, link);
  hipLaunchKernelGGL(mk_gb_decode_kernel, dim3(waves), dim3(64 * MK_INFL_WAVES), 0, s, d_comp, blks, d_ftab, n, pieces, nspans, d_syms);
  hipLaunchKernelGGL(mk_gb_chain_kernel, dim3(n), dim3(1024), 0, s, blks, d_ftab, n, pieces, link, (const uint16_t *)d_syms, d_win, d_work);
  /* blocks a piece: one per 16 KiB of text it may give at a ratio of four */
  const uint32_t per = g.S / 4096u < 1u ? 1u : g.S / 4096u > 64u ? 64u : g.S / 4096u;
  hipLaunchKernelGGL(mk_gb_resolve_kernel, dim3(per, nspans), dim3(256), 0, s, (const mk_gun_piece *)pieces, (const mk_gb_link *)link, (const uint16_t *)d_syms,
                     (const uint8_t *)d_win, d_text);
  if (nslices) hipLaunchKernelGGL(mk_crc32_files_kernel, dim3((nslices + 3u) / 4u), dim3(256), 0, s, (const uint8_t *)d_text, blks, slice0s, n, nslices, slice_crc);
  hipLaunchKernelGGL(mk_crc32_combine_kernel, dim3((n + 63u) / 64u), dim3(64), 0, s, blks, slice0s, n, (const uint32_t *)slice_crc, d_work, d_work + 3u * (size_t)n);
  return hipGetLastError();
}

/* mk_inflate_members through the kernels above, with the piece lists (tests, tools) */
extern "C" int mk_inflate_members_split(mk_inflate *h, const uint8_t *comp, size_t comp_bytes, const mk_gz_member *members, uint32_t nmembers,
                                        const mk_gunzip_opts *opts, uint8_t *out_host, size_t out_cap, mk_gz_member_result *res,
                                        mk_gunzip_pieces *pieces_per_member) {
  if (!h || (!comp && comp_bytes) || (!members && nmembers) || !res) return MK_ERR_ARG;
  for (uint32_t i = 0; i < nmembers && pieces_per_member; i++) { pieces_per_member[i].v = nullptr; pieces_per_member[i].n = 0; }
  if (nmembers == 0) return MK_OK;
  mk_gb_geom G;
  if (!mk_gb_geometry(opts, &G)) return mk_infl_fail(h, MK_ERR_ARG, "mk_inflate_members_split: flags must be 0 (a concatenation of members is MK_INFL_TRAILING here)");
  if (nmembers > (1u << 20) || comp_bytes >= (1ull << 31)) return mk_infl_fail(h, MK_ERR_ARG, "mk_inflate_members_split: at most 2^20 members and 2 GiB a call");
  uint64_t text_end = 0, nslices = 0;
  for (uint32_t i = 0; i < nmembers; i++) {
    const mk_gz_member &m = members[i];
    if (m.pay_off + (uint64_t)m.pay_len > comp_bytes || m.isize > MK_BATCH_FILE_MAX || m.out_off + m.isize > (1ull << 30))
      return mk_infl_fail(h, MK_ERR_ARG, "mk_inflate_members_split: member %u lies outside the buffers", i);
    if (m.out_off + m.isize > text_end) text_end = m.out_off + m.isize;
    nslices += mk_gz_slices(m.isize);
  }
  if (out_host && out_cap < text_end) return mk_infl_fail(h, MK_ERR_ARG, "mk_inflate_members_split: out_cap too small");
  MK_INFL_HIP(h, hipSetDevice(h->device));
  /* one upload: the payloads | the member table | the span table of the files */
  const uint64_t tab_at = (comp_bytes + 15u) & ~(uint64_t)15u, ftab_at = tab_at + mk_gz_table_bytes(nmembers);
  const uint64_t stage_bytes = ftab_at + (uint64_t)nmembers * sizeof(mk_gb_file);
  MK_INFL_HIP(h, mk_grow(&h->h_stage, &h->stage_cap, stage_bytes, true));
  if (comp_bytes) memcpy(h->h_stage, comp, comp_bytes);
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
  mk_gb_file *ftab = (mk_gb_file *)(h->h_stage + ftab_at);
  uint64_t nspans = 0, nsyms = 0;
  if (!mk_gb_plan(tab, nmembers, G, ftab, &nspans, &nsyms))
    return mk_infl_fail(h, MK_ERR_ARG, "mk_inflate_members_split: %llu spans and %llu symbols (at most %u and %llu a call)", (unsigned long long)nspans,
                        (unsigned long long)nsyms, MK_GB_SPANS_MAX, (unsigned long long)MK_GB_SYMS_MAX);
  struct bufs { /* what only this call needs */
    uint8_t *d_scratch = nullptr, *d_win = nullptr, *h_scratch = nullptr;
    uint16_t *d_syms = nullptr;
    ~bufs() { (void)hipFree(d_scratch); (void)hipFree(d_win); (void)hipFree(d_syms); if (h_scratch) (void)hipHostFree(h_scratch); }
  } B;
  const uint64_t words = mk_gb_work_words(nmembers, (uint32_t)nslices);
  const size_t scratch_bytes = mk_gb_scratch_bytes(nspans);
  MK_INFL_HIP(h, mk_grow(&h->d_comp, &h->comp_cap, stage_bytes + 64, false));
  MK_INFL_HIP(h, mk_grow(&h->d_text, &h->text_cap, mk_fq_buf_bytes(text_end), false));
  MK_INFL_HIP(h, mk_grow(&h->d_status, &h->status_cap, words, false));
  MK_INFL_HIP(h, mk_grow(&h->h_status, &h->h_status_cap, 5u * (uint64_t)nmembers, true));
  MK_INFL_HIP(h, mk_dev_alloc(&B.d_scratch, scratch_bytes));
  MK_INFL_HIP(h, mk_dev_alloc(&B.d_win, mk_gb_win_bytes(nspans)));
  MK_INFL_HIP(h, mk_dev_alloc(&B.d_syms, mk_gb_sym_bytes(nsyms)));
  MK_INFL_HIP(h, mk_pin_alloc(&B.h_scratch, scratch_bytes, hipHostMallocDefault));
  MK_INFL_HIP(h, hipMemcpyAsync(h->d_comp, h->h_stage, stage_bytes, hipMemcpyHostToDevice, h->stream));
  if (out_host && text_end) MK_INFL_HIP(h, hipMemcpyAsync(h->d_text, out_host, text_end, hipMemcpyHostToDevice, h->stream)); /* what no piece writes comes back as it was */
  MK_INFL_HIP(h, hipEventRecord(h->ev[0], h->stream));
  MK_INFL_HIP(h, mk_gb_launch(h->stream, h->d_comp, h->d_comp + tab_at, (const mk_gb_file *)(h->d_comp + ftab_at), nmembers, s0, (uint32_t)nspans, G, B.d_scratch,
                              B.d_syms, B.d_win, h->d_text, h->d_status));
  MK_INFL_HIP(h, hipEventRecord(h->ev[1], h->stream));
  MK_INFL_HIP(h, hipMemcpyAsync(h->h_status, h->d_status, 5u * (size_t)nmembers * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  MK_INFL_HIP(h, hipMemcpyAsync(B.h_scratch, B.d_scratch, scratch_bytes, hipMemcpyDeviceToHost, h->stream));
  MK_INFL_HIP(h, hipStreamSynchronize(h->stream));
  for (uint32_t i = 0; i < nmembers; i++)
    res[i] = mk_gz_member_result{h->h_status[i], h->h_status[nmembers + i], h->h_status[2u * (size_t)nmembers + i], h->h_status[3u * (size_t)nmembers + i]};
  if (out_host && text_end) MK_INFL_HIP(h, hipMemcpy(out_host, h->d_text, text_end, hipMemcpyDeviceToHost));
  float ms = 0.f;
  MK_INFL_HIP(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  h->inflate_ms = ms;
  if (pieces_per_member) {
    const mk_gun_piece *P = (const mk_gun_piece *)(B.h_scratch + mk_gb_pieces_at(nspans));
    for (uint32_t i = 0; i < nmembers; i++) {
      const uint32_t np = h->h_status[4u * (size_t)nmembers + i];
      if (np > ftab[i].nspans) return mk_infl_fail(h, MK_ERR_HIP, "mk_inflate_members_split: member %u reports more pieces than it has spans", i);
      mk_gunzip_piece *v = (mk_gunzip_piece *)malloc((size_t)(np ? np : 1u) * sizeof(mk_gunzip_piece));
      if (!v) return MK_ERR_NOMEM;
      uint32_t k = 0;
      for (uint32_t c = 0; c < ftab[i].nspans && k < np; c++) {
        const mk_gun_piece &p = P[ftab[i].span0 + c];
        if (p.start != MK_GUN_NONE) v[k++] = mk_gunzip_piece{p.start, p.len};
      }
      pieces_per_member[i].v = v;
      pieces_per_member[i].n = k;
    }
  }
  return MK_OK;
}
