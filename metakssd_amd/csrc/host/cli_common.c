/* cli_common.c -- helpers every command of the `metakssd` command line uses: die(), input discovery, whole-file reads, and the one
 * reader of a sketch directory's cofiles.stat / a database's mcofiles.stat. */
#include "cli.h"

void die(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "metakssd: ");
  vfprintf(stderr, fmt, ap);
  fprintf(stderr, "\n");
  va_end(ap);
  /* not exit(): with driver / worker threads still inside HIP calls the runtime's exit handlers can wait for them forever */
  fflush(NULL);
  _exit(1);
}
int has_suffix(const char *s, const char *suf) {
  size_t a = strlen(s), b = strlen(suf);
  return a >= b && strcmp(s + a - b, suf) == 0;
}
/* isOK_fmt_infile(): one optional .gz/.bz2, then the format suffix (global_basic.h:162-186, global_basic.c:96-128) */
static int fmt_match(const char *name, const char *const *fmts, int n) {
  char tmp[PATHLEN * 2];
  snprintf(tmp, sizeof tmp, "%s", name);
  if (has_suffix(tmp, ".gz")) tmp[strlen(tmp) - 3] = 0;
  else if (has_suffix(tmp, ".bz2")) tmp[strlen(tmp) - 4] = 0;
  for (int i = 0; i < n; i++) {
    char suf[16];
    snprintf(suf, sizeof suf, ".%s", fmts[i]);
    if (has_suffix(tmp, suf)) return 1;
  }
  return 0;
}
static const char *const FASTA_FMT[] = {"fasta", "fna", "fas", "fa"};
static const char *const FASTQ_FMT[] = {"fq", "fastq"};
int is_fastq(const char *n) { return fmt_match(n, FASTQ_FMT, 2); }
int is_fasta(const char *n) { return fmt_match(n, FASTA_FMT, 4); }
int is_compressed(const char *n) { return has_suffix(n, ".gz") || has_suffix(n, ".bz2"); }

void sl_push(strlist *l, const char *s) {
  if (strlen(s) >= PATHLEN) die("path: %s exceed maximal path lenth %d", s, PATHLEN);
  if (l->n == l->cap) { l->cap = l->cap ? l->cap * 2 : 64; l->v = realloc(l->v, sizeof(char *) * l->cap); }
  l->v[l->n++] = strdup(s);
}
static int cmp_str(const void *a, const void *b) { return strcmp(*(char *const *)a, *(char *const *)b); }

/* organize_infile_frm_arg(): global_basic.c:246-325 (directories expanded one level; here sorted by name) */
void discover(strlist *out, int argc, char **argv) {
  for (int i = 0; i < argc; i++) {
    struct stat st;
    if (stat(argv[i], &st) != 0) die("%dth argument: can't open %s", i + 1, argv[i]);
    if (S_ISDIR(st.st_mode)) {
      DIR *d = opendir(argv[i]);
      if (!d) die("%dth argument: can't open %s", i + 1, argv[i]);
      strlist tmp = {0};
      struct dirent *de;
      while ((de = readdir(d)) != NULL) {
        char full[PATHLEN * 4];
        snprintf(full, sizeof full, "%s/%s", argv[i], de->d_name);
        if (is_fastq(full) || is_fasta(full)) sl_push(&tmp, full);
      }
      closedir(d);
      qsort(tmp.v, tmp.n, sizeof(char *), cmp_str);
      for (int j = 0; j < tmp.n; j++) { sl_push(out, tmp.v[j]); free(tmp.v[j]); }
      free(tmp.v);
    } else if (is_fastq(argv[i]) || is_fasta(argv[i])) {
      sl_push(out, argv[i]);
    } else {
      die("wrong format %dth argument: %s (supported: .fna .fas .fasta .fq .fastq .fa, optionally .gz/.bz2)", i + 1, argv[i]);
    }
  }
}
double now_s(void) {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec + 1e-9 * ts.tv_nsec;
}
uint8_t *read_whole(const char *path, size_t *n_out) {
  struct stat st;
  if (stat(path, &st) != 0) return NULL;
  FILE *f = fopen(path, "rb");
  if (!f) return NULL;
  uint8_t *b = malloc((size_t)st.st_size + 8);
  if (b && fread(b, 1, (size_t)st.st_size, f) != (size_t)st.st_size) { free(b); b = NULL; }
  fclose(f);
  *n_out = (size_t)st.st_size;
  return b;
}
void *map_whole(const char *path, size_t *n) {
  int fd = open(path, O_RDONLY);
  if (fd < 0) return NULL;
  struct stat st;
  if (fstat(fd, &st) != 0) { close(fd); return NULL; }
  *n = (size_t)st.st_size;
  void *p = st.st_size ? mmap(NULL, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0) : NULL;
  close(fd);
  return p == MAP_FAILED ? NULL : p;
}
int dir_has(const char *dir, const char *name) { /* test_get_fullpath(), command_dist.c:318-338 */
  char path[PATHLEN * 2 + 32];
  struct stat st;
  if (stat(dir, &st) != 0 || !S_ISDIR(st.st_mode)) return 0;
  snprintf(path, sizeof path, "%s/%s", dir, name);
  FILE *f = fopen(path, "rb");
  if (!f) return 0;
  fclose(f);
  return 1;
}
/* the .shuf file of -L and the geometry it gives at --component-sz */
void load_shuf_params(const char *shuf_path, mk_shuf *sh, mk_params *P) {
  if (!shuf_path) die("-L <file.shuf> is required");
  int rc = mk_shuf_read(shuf_path, sh);
  if (rc != MK_OK) die("read_dim_shuffle_file(): cannot read %s (%d)", shuf_path, rc);
  rc = mk_params_init_csz(sh, g_opt.component_sz, P);
  if (rc == MK_ERR_ARG) die("--component-sz %d with k=%d drlevel=%d: more than 16 components (or out of 1..8)", g_opt.component_sz, sh->k, sh->drlevel);
  if (rc != MK_OK) die("get_hashsz(): primer_ind out of range(0 ~ 24) for k=%d drlevel=%d (command_dist.c:291-303)", sh->k, sh->drlevel);
}
uint8_t *read_part(char *path, size_t cap, const char *dir, const char *stem, int c, size_t need, size_t *n_out) {
  snprintf(path, cap, "%s/%s.%d", dir, stem, c);
  uint8_t *b = read_whole(path, n_out);
  if (b && *n_out < need) { free(b); b = NULL; }
  return b;
}
uint8_t *need_part(const char *who, const char *dir, const char *stem, int c, size_t need, size_t *n_out) {
  char path[PATHLEN * 4 + 64];
  uint8_t *b = read_part(path, sizeof path, dir, stem, c, need, n_out);
  if (!b) die("%s%s", who, path);
  return b;
}
/* ---- the header of a sketch directory and of a database, decoded HERE and nowhere else ----------------------------------------
 * cofiles.stat is a co_dstat_t (global_basic.h:116-126): shuf_id u32 at 0, koc (bool) at 4, kmerlen i32 at 8, dim_rd_len at 12,
 * comp_num at 16, infile_num at 20, all_ctx_ct u64 at 24 -- 32 bytes -- then infile_num u32 k-mer counts and infile_num names of
 * PATHLEN bytes (mk_sketchdir.c writes it).  mcofiles.stat is an mco_dstat_t (command_dist.h:66-75): shuf_id at 0, kmerlen at 4,
 * dim_rd_len at 8, comp_num at 12, infile_num at 16 -- 20 bytes -- then the same counts and names (run_stage2 writes it). */
static int stat_load(const char *dir, const char *name, size_t hdr, costat *s) {
  memset(s, 0, sizeof *s);
  snprintf(s->path, sizeof s->path, "%s/%s", dir, name);
  s->raw = read_whole(s->path, &s->n);
  s->hdr = hdr;
  if (!s->raw || s->n < hdr) return COSTAT_ABSENT;
  const uint8_t *f = s->raw + (hdr == 32 ? 8 : 4); /* kmerlen, dim_rd_len, comp_num, infile_num lie side by side in both */
  memcpy(&s->shuf_id, s->raw, 4);
  memcpy(&s->kmerlen, f, 4); memcpy(&s->dim_rd_len, f + 4, 4); memcpy(&s->comp_num, f + 8, 4); memcpy(&s->infile_num, f + 12, 4);
  if (hdr == 32) { s->koc = s->raw[4]; memcpy(&s->all_ctx_ct, s->raw + 24, 8); }
  s->ctx_ct = (uint32_t *)(s->raw + hdr);
  s->names = (const char *)s->raw + hdr + 4 * (size_t)s->infile_num;
  if (s->n >= hdr + (size_t)s->infile_num * (4 + PATHLEN)) return COSTAT_FULL;
  return s->n >= hdr + 4 * (size_t)s->infile_num ? COSTAT_COUNTS : COSTAT_HEADER;
}
int costat_load(const char *dir, costat *s) { return stat_load(dir, "cofiles.stat", 32, s); }
int mcostat_load(const char *dir, costat *s) { return stat_load(dir, "mcofiles.stat", 20, s); }
/* for who writes a cofiles.stat header back with other totals: the 32 bytes at raw, the rest of them as they were */
void costat_set_totals(costat *s, int32_t infile_num, int koc, uint64_t all_ctx_ct) {
  s->infile_num = infile_num; s->koc = koc; s->all_ctx_ct = all_ctx_ct;
  memcpy(s->raw + 20, &infile_num, 4);
  s->raw[4] = (uint8_t)koc;
  memcpy(s->raw + 24, &all_ctx_ct, 8);
}
