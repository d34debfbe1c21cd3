/*
 * mk_byread_files.c -- the file side of `dist --byread` and `reverse` that is no id stream (host C, no GPU).
 *
 * mk_byread_write_stat: the cofiles.stat record run_stageI() writes behind reads2mco() (command_dist.c:477-500): the co_dstat_t
 * header with infile_num 1 and all_ctx_ct 0, one ctx_ct word and the input's path in PATHLEN bytes.  The reference never
 * initialises that ctx_ct word (nothing counts in the by-read branch, :353-360); here it is 0, like the padding.
 * mk_reverse_outname: the name co_reverse2kmer() gives a sketch's k-mer file (command_reverse.c:335-337): the basename of the
 * recorded path with every ' ' replaced by '_'.
 */
#include "metakssd_hip.h"

#include <stdio.h>
#include <string.h>

#define MK_PATHLEN 256 /* global_basic.h:32 */

int mk_byread_write_stat(const char *outdir, const mk_params *p, const char *input_path) {
  if (!outdir || !p || !input_path || strlen(input_path) >= MK_PATHLEN || strlen(outdir) > 1024) return MK_ERR_ARG;
  unsigned char rec[32 + 4 + MK_PATHLEN]; /* co_dstat_t laid out by hand: offsets 0,4,8,12,16,20,24 */
  memset(rec, 0, sizeof rec);
  const uint32_t id = (uint32_t)p->shuf_id;
  const int32_t kmerlen = p->k * 2, dim_rd_len = p->drlevel * 2, comp_num = p->component_num, infile_num = 1;
  memcpy(rec + 0, &id, 4);
  memcpy(rec + 8, &kmerlen, 4);
  memcpy(rec + 12, &dim_rd_len, 4);
  memcpy(rec + 16, &comp_num, 4);
  memcpy(rec + 20, &infile_num, 4);
  strcpy((char *)rec + 36, input_path);
  char path[1100];
  snprintf(path, sizeof path, "%s/cofiles.stat", outdir);
  FILE *f = fopen(path, "wb");
  if (!f) return MK_ERR_IO;
  int rc = fwrite(rec, 1, sizeof rec, f) == sizeof rec ? MK_OK : MK_ERR_IO;
  if (fclose(f) != 0) rc = MK_ERR_IO;
  return rc;
}

int mk_reverse_outname(const char *recorded_path, char *out, size_t cap) {
  if (!recorded_path || !out || cap < 2) return MK_ERR_ARG;
  char tmp[MK_PATHLEN + 1];
  memcpy(tmp, recorded_path, MK_PATHLEN); /* the field of cofiles.stat need not be terminated */
  tmp[MK_PATHLEN] = 0;
  const char *base = strrchr(tmp, '/');
  base = base ? base + 1 : tmp;
  if (!*base || strlen(base) >= cap) return MK_ERR_ARG;
  size_t i = 0;
  for (; base[i]; i++) out[i] = base[i] == ' ' ? '_' : base[i];
  out[i] = 0;
  return MK_OK;
}
