/* cli_byread.c -- `dist -L <.shuf> --byread -o <out> <file>` (reads2mco(), iseq2comem.c:88-214: per-record id streams of ONE plain-text
 * file) and `reverse -L <.shuf> [-o outdir] [-p N] [-b] <dir>` (command_reverse.c:148-353: ids back to k-mers, per sketch into files
 * or, -b, per read to stdout).  mk_byread_*: the device does the walk, the compaction and the formatting. */
#include "cli.h"

static void byread_die(mk_byread *b, const char *what, int rc) { die("%s: %s (%d)", what, mk_byread_last_error(b), rc); }

/* run_stageI() with opt_val->byread (command_dist.c:353-360) + reads2mco() + the cofiles.stat record (:477-500) */
int cmd_dist_byread(int argc, char **argv) {
  const char *shuf_path = NULL, *outdir = ".";
  int device = 0, quiet = 0;
  strlist args = {0};
  for (int i = 0; i < argc; i++) {
    if (!strcmp(argv[i], "--byread")) continue;
    else if (!strcmp(argv[i], "-L") && i + 1 < argc) shuf_path = argv[++i];
    else if (!strcmp(argv[i], "-o") && i + 1 < argc) outdir = argv[++i];
    else if (!strcmp(argv[i], "-p") && i + 1 < argc) ++i; /* threads: one file, one walk */
    else if (!strcmp(argv[i], "--device") && i + 1 < argc) device = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--quiet")) quiet = 1;
    else if (!strcmp(argv[i], "--component-sz") && i + 1 < argc) g_opt.component_sz = atoi(argv[++i]);
    else if (!strcmp(argv[i], "-A") || !strcmp(argv[i], "-u") || !strcmp(argv[i], "-n") || !strcmp(argv[i], "-Q") || !strcmp(argv[i], "--devices"))
      die("%s cannot be combined with --byread (every accepted k-mer of one file is kept, on one GPU)", argv[i]);
    else if (argv[i][0] == '-' && argv[i][1]) die("option %s cannot be combined with --byread", argv[i]);
    else sl_push(&args, argv[i]);
  }
  if (args.n != 1) die("--byread takes exactly one input file (got %d): the reference overwrites combco.* file after file", args.n);
  const char *in = args.v[0];
  struct stat st;
  if (stat(in, &st) != 0 || !S_ISREG(st.st_mode)) die("1th argument: can't open %s", in);
  if (!is_fastq(in) && !is_fasta(in)) die("wrong format 1th argument: %s (supported: .fna .fas .fasta .fq .fastq .fa)", in);
  if (is_compressed(in)) die("--byread reads plain text: decompress %s first", in);
  mk_shuf sh;
  mk_params P;
  load_shuf_params(shuf_path, &sh, &P);
  if (!quiet) printf("rand_id=%d\thalf_ctx_len=%d\thashsize=%u\thashlimit=%u\n", P.shuf_id, P.k, P.hashsize, P.hashlimit);
  mk_byread *b = NULL;
  int rc = mk_byread_create(device, &b);
  if (rc != MK_OK) byread_die(NULL, "mk_byread_create", rc);
  if ((rc = mk_byread_begin(b, &P)) != MK_OK) byread_die(b, "mk_byread_begin", rc);
  if (mkdir(outdir, 0777) != 0 && errno != EEXIST) die("%s: %s", outdir, strerror(errno));
  const int C = P.component_num;
  FILE *fid[16], *fix[16];
  char path[PATHLEN * 4 + 64];
  for (int c = 0; c < C; c++) {
    snprintf(path, sizeof path, "%s/combco.%d", outdir, c);
    if (!(fid[c] = fopen(path, "wb"))) die("%s: %s", path, strerror(errno));
    snprintf(path, sizeof path, "%s/combco.index.%d", outdir, c);
    if (!(fix[c] = fopen(path, "wb"))) die("%s: %s", path, strerror(errno));
  }
  FILE *f = fopen(in, "rb");
  if (!f) die("reads2mco():%s: %s", in, strerror(errno));
  printf("decomposing %s by reads\n", in);
  uint8_t *buf = malloc(MK_BYREAD_MAX_PUSH);
  if (!buf) die("out of memory");
  for (int final = 0; !final;) {
    const size_t n = fread(buf, 1, MK_BYREAD_MAX_PUSH, f);
    if (ferror(f)) die("reads2mco():%s: read error", in);
    final = n < MK_BYREAD_MAX_PUSH;
    rc = mk_byread_push_text(b, buf, n, final);
    if (rc == MK_ERR_FORMAT) die("fasta2co(): can not find seqences head start from '>' (%s ends inside a header line)", in);
    if (rc != MK_OK) byread_die(b, "mk_byread_push_text", rc);
    for (int c = 0; c < C; c++) {
      const uint32_t *ids; const uint64_t *idx; uint64_t nid, nix;
      if ((rc = mk_byread_take(b, (uint32_t)c, &ids, &nid, &idx, &nix)) != MK_OK) byread_die(b, "mk_byread_take", rc);
      if (nid && fwrite(ids, 4, nid, fid[c]) != nid) die("combco.%d: write error", c);
      if (nix && fwrite(idx, 8, nix, fix[c]) != nix) die("combco.index.%d: write error", c);
    }
  }
  fclose(f);
  free(buf);
  for (int c = 0; c < C; c++)
    if (fclose(fid[c]) != 0 || fclose(fix[c]) != 0) die("combco.%d: write error", c);
  if ((rc = mk_byread_finish(b, NULL, NULL, NULL)) != MK_OK) byread_die(b, "mk_byread_finish", rc);
  if ((rc = mk_byread_write_stat(outdir, &P, in)) != MK_OK) die("%s/cofiles.stat: cannot write (%d)", outdir, rc);
  printf("decomposing %s by reads is complete!\n", in);
  mk_byread_destroy(b);
  return 0;
}
typedef struct { /* one component's ids behind `reverse -b`'s cursor, a batch at a time */
  FILE *f;
  uint32_t *ids;
  char *text;
  uint64_t lo, hi; /* ids [lo, hi) of the file are in text */
} rvs_comp;
#define RVS_BATCH ((uint64_t)1 << 20)

int cmd_reverse(int argc, char **argv) {
  const char *shuf_path = NULL, *outdir = ".", *dir = NULL;
  int device = 0, byreads = 0, ndirs = 0;
  for (int i = 0; i < argc; i++) {
    if (!strcmp(argv[i], "-L") && i + 1 < argc) shuf_path = argv[++i];
    else if (!strcmp(argv[i], "-o") && i + 1 < argc) outdir = argv[++i];
    else if (!strcmp(argv[i], "-p") && i + 1 < argc) ++i; /* threads of the reference's loops: the device formats */
    else if (!strcmp(argv[i], "-b")) byreads = 1;
    else if (!strcmp(argv[i], "--device") && i + 1 < argc) device = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--component-sz") && i + 1 < argc) g_opt.component_sz = atoi(argv[++i]);
    else if (argv[i][0] == '-' && argv[i][1]) die("reverse: unknown option %s", argv[i]);
    else { dir = argv[i]; ndirs++; }
  }
  if (ndirs != 1) die("need speficy one query path");
  struct stat st;
  if (stat(dir, &st) != 0 || !S_ISDIR(st.st_mode) || !dir_has(dir, "cofiles.stat")) die("%s is not a valid query folder", dir);
  if (!byreads && (stat(outdir, &st) != 0 || !S_ISDIR(st.st_mode))) die("reverse: the output directory %s does not exist", outdir);
  mk_shuf sh;
  mk_params P;
  load_shuf_params(shuf_path, &sh, &P);
  {
    int count = 0;
    for (uint64_t i = 0; i < sh.len; i++) count += sh.table[i] >= 0 && sh.table[i] < 4096;
    if (count != 4096) die("count %d not match MIN_SUBCTX_DIM_SMP_SZ 4096: %s cannot be inverted", count, shuf_path);
  }
  char path[PATHLEN * 4 + 64];
  costat s;
  const int have = costat_load(dir, &s);
  if (have == COSTAT_ABSENT) die("qry co stat file:%s", s.path);
  const int32_t comp_num = s.comp_num, infile_num = s.infile_num;
  if (comp_num != P.component_num) die("%s has %d components, %s gives %d", dir, comp_num, shuf_path, P.component_num);
  if (infile_num < 0 || have < COSTAT_FULL) die("qry co stat file:%s is truncated", s.path);
  mk_byread *b = NULL;
  int rc = mk_byread_create(device, &b);
  if (rc != MK_OK) byread_die(NULL, "mk_byread_create", rc);
  if ((rc = mk_byread_begin(b, &P)) != MK_OK) byread_die(b, "mk_byread_begin", rc);
  const uint64_t W = (uint64_t)P.TL + 1;
  if (byreads) { /* co_rvs2kmer_byreads(), command_reverse.c:148-232 */
    snprintf(path, sizeof path, "%s/combco.index.0", dir);
    if (stat(path, &st) != 0) die("co_rvs2kmer_btreads()::%s", path);
    const uint64_t readn = (uint64_t)st.st_size / 8 ? (uint64_t)st.st_size / 8 - 1 : 0;
    uint64_t **index = calloc((size_t)comp_num, sizeof *index);
    rvs_comp *rc_ = calloc((size_t)comp_num, sizeof *rc_);
    for (int c = 0; c < comp_num; c++) {
      size_t n = 0;
      index[c] = (uint64_t *)need_part("co_rvs2kmer_btreads()::", dir, "combco.index", c, 8 * (size_t)(readn + 1), &n);
      snprintf(path, sizeof path, "%s/combco.%d", dir, c);
      if (!(rc_[c].f = fopen(path, "rb"))) die("co_rvs2kmer_btreads()::%s", path);
      rc_[c].ids = malloc(RVS_BATCH * 4);
      rc_[c].text = malloc(RVS_BATCH * W);
      if (!rc_[c].ids || !rc_[c].text) die("out of memory");
    }
    static char obuf[1 << 22];
    setvbuf(stdout, obuf, _IOFBF, sizeof obuf);
    for (uint64_t n = 0; n < readn; n++) {
      printf(">read %llu\n", (unsigned long long)(n + 1));
      for (int c = 0; c < comp_num; c++) {
        rvs_comp *k = &rc_[c];
        /* the cursor starts at the beginning of the component's file, whatever index[0] says (command_reverse.c:212-213) */
        uint64_t cur = index[c][n] - index[c][0], end = index[c][n + 1] - index[c][0];
        while (cur < end) {
          if (cur >= k->hi) {
            const size_t got = fread(k->ids, 4, RVS_BATCH, k->f);
            if (!got) die("co_rvs2kmer_btreads()::combco.%d is shorter than its index", c);
            k->lo = k->hi; k->hi += got;
            if ((rc = mk_reverse_ids(b, k->ids, got, (uint32_t)c, k->text)) != MK_OK) byread_die(b, "mk_reverse_ids", rc);
          }
          const uint64_t upto = end < k->hi ? end : k->hi;
          fwrite(k->text + (cur - k->lo) * W, 1, (upto - cur) * W, stdout);
          cur = upto;
        }
      }
    }
    fflush(stdout);
    mk_byread_destroy(b);
    return 0;
  }
  /* co_reverse2kmer(), command_reverse.c:237-353: component by component, every sketch's block appended to its file */
  uint64_t *written = calloc((size_t)infile_num + 1, sizeof *written);
  for (int c = 0; c < comp_num; c++) {
    size_t nb = 0, xb = 0;
    uint32_t *ids = (uint32_t *)need_part("co_reverse2kmer()::", dir, "combco", c, 0, &nb);
    uint64_t *pos = (uint64_t *)need_part("co_reverse2kmer()::", dir, "combco.index", c, 8 * ((size_t)infile_num + 1), &xb);
    const uint64_t n = nb / 4;
    if (pos[infile_num] > n) die("co_reverse2kmer()::combco.%d is shorter than its index", c);
    char *text = malloc(n * W + 1);
    if (!text) die("out of memory");
    if ((rc = mk_reverse_ids(b, ids, n, (uint32_t)c, text)) != MK_OK) byread_die(b, "mk_reverse_ids", rc);
    for (int k = 0; k < infile_num; k++) {
      const uint32_t ct = s.ctx_ct[k];
      if (ct == 0) continue; /* :331: no file for a sketch without ids */
      char name[PATHLEN + 1];
      if (mk_reverse_outname(s.names + (size_t)PATHLEN * k, name, sizeof name) != MK_OK) die("bad name in cofiles.stat");
      snprintf(path, sizeof path, "%s/%s", outdir, name);
      FILE *o = fopen(path, c == 0 ? "w" : "a");
      if (!o) die("%s: %s", path, strerror(errno));
      uint64_t m = pos[k + 1] - pos[k];
      if (written[k] + m > ct) m = ct - written[k]; /* :342: ctx_ct lines are printed */
      if (m && fwrite(text + pos[k] * W, 1, m * W, o) != m * W) die("%s: write error", path);
      if (fclose(o) != 0) die("%s: write error", path);
      written[k] += m;
    }
    free(text); free(ids); free(pos);
  }
  mk_byread_destroy(b);
  return 0;
}
