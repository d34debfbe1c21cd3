/* cli_composite.c -- `metakssd composite`: -r -q [-b], -d, -i, -s (command_composite.c) */
#include "cli.h"

/* ---- `metakssd composite -r <ref> -q <qry> [-b] [-o outdir]`: get_species_abundance(), command_composite.c:446-649 ----
 * The join (query k-mer dictionary, lookup of every reference k-mer, :525-553) runs on the device, one mk_setop_join per
 * query and component; the order statistics over each reference's handful of counts and the report stay on the host,
 * in the reference's float arithmetic. */
static int cmp_int_asc(const void *a, const void *b) { return *(const int *)a - *(const int *)b; }

/* `composite -d <x.abv>...`: read_abv(), command_composite.c:186-210 -- prints the (reference index, percentage) pairs of
 * the vector files `composite -b` writes.  Host only. */
static int composite_read_abv(int nfiles, char **files) {
  for (int i = 0; i < nfiles; i++) {
    const char *ext = strrchr(files[i], '.');
    if (!ext || strcmp(ext + 1, "abv") != 0) {
      printf("%dth argument %s is not a .abv file, skipped\n", i, files[i]);
      continue;
    }
    size_t n = 0;
    uint8_t *b = read_whole(files[i], &n);
    if (!b) die("read_abv():%s", files[i]);
    for (size_t l = 0; l + 8 <= n || l < n; l += 8) { /* the reference loops while l < st_size */
      int32_t idx = 0;
      float pct = 0;
      if (l + 8 <= n) { memcpy(&idx, b + l, 4); memcpy(&pct, b + l + 4, 4); }
      printf("%d\t%f\n", idx, pct);
    }
    free(b);
  }
  return 1;
}
/* ---- `composite -r <ref> -i` / `composite -r <ref> -s <0|1|2> <x.abv>...`: index_abv() and abv_search(),
 * command_composite.c:347-440 and :212-344.  The index (a stable sort by species) and the search (accumulation, ordering)
 * run on the device (mk_abv_*); reading the files and printing stay here. */
static int abv_name_ok(const char *name) { /* strrchr(name,'.') + 1 == "abv"; a name without a dot crashes the reference */
  const char *ext = strrchr(name, '.');
  return ext && strcmp(ext + 1, "abv") == 0;
}
static int composite_index(const char *refdir, int device) {
  char dpath[PATHLEN * 2 + 32], path[PATHLEN * 3 + 64];
  snprintf(dpath, sizeof dpath, "%s/abundance_Vec", refdir);
  DIR *dir = opendir(dpath);
  if (!dir) die("index_abv(): %s does not exists! ", dpath);
  costat s;
  if (costat_load(refdir, &s) == COSTAT_ABSENT) die("cannot find cofiles.stat under %s ", refdir);
  const int32_t nref = s.infile_num;
  free(s.raw);
  if (nref < 0) die("index_abv(): %s: infile_num %d", s.path, nref);
  /* readdir order, unsorted, as the reference walks it (:379) */
  size_t nf = 0, fcap = 64, ncap = 1 << 16, nlen = 0, ecap = 1 << 16;
  uint64_t n = 0, *fend = malloc(8 * fcap);
  char *names = malloc(ncap);
  mk_binvec *ent = malloc(sizeof(mk_binvec) * ecap);
  struct dirent *de;
  while ((de = readdir(dir)) != NULL) {
    if (!abv_name_ok(de->d_name)) continue;
    snprintf(path, sizeof path, "%s/%s", dpath, de->d_name);
    struct stat fs;
    FILE *f = fopen(path, "rb");
    if (!f || fstat(fileno(f), &fs) != 0) die("index_abv():%s", path);
    const uint64_t len = (uint64_t)fs.st_size / sizeof(mk_binvec);
    if (n + len > 0x7FFFFFFFull) die("index_abv(): more than 2^31-1 entries (.abmi holds int32 counts)");
    if (n + len > ecap) {
      while (n + len > ecap) ecap *= 2;
      ent = realloc(ent, sizeof(mk_binvec) * ecap);
    }
    if (len && fread(ent + n, sizeof(mk_binvec), len, f) != len) die("index_abv():%s", path);
    fclose(f);
    n += len;
    if (nf == fcap) { fcap *= 2; fend = realloc(fend, 8 * fcap); }
    fend[nf++] = n;
    const size_t l = strlen(de->d_name);
    if (nlen + l + 2 > ncap) { while (nlen + l + 2 > ncap) ncap *= 2; names = realloc(names, ncap); }
    memcpy(names + nlen, de->d_name, l);
    names[nlen + l] = '\n';
    nlen += l + 1;
  }
  closedir(dir);
  if (!ent || !fend || !names) die("index_abv(): out of memory");
  mk_abv *a;
  if (mk_abv_create(device, &a) != MK_OK) die("mk_abv_create failed: %s", mk_abv_last_error(NULL));
  const mk_binvec *abm;
  const int32_t *abmi;
  const double *yl2n;
  int64_t bad = -1;
  if (mk_abv_index(a, ent, n, fend, (uint32_t)nf, (uint32_t)nref, &abm, &abmi, &yl2n, &bad) != MK_OK) {
    if (bad >= 0) { /* the bad_file-th name */
      const char *nm = names;
      for (int64_t k = 0; k < bad; k++) nm = strchr(nm, '\n') + 1;
      die("index_abv(): %s/%.*s: %s", dpath, (int)(strchr(nm, '\n') - nm), nm, mk_abv_last_error(a));
    }
    die("index_abv(): %s", mk_abv_last_error(a));
  }
  static const char *suf[4] = {"name", "yl2n", "abm", "abmi"};
  const void *data[4] = {names, yl2n, abm, abmi};
  const size_t bytes[4] = {nlen, 8 * nf, sizeof(mk_binvec) * n, 4 * (size_t)nref};
  for (int k = 0; k < 4; k++) {
    snprintf(path, sizeof path, "%s/abundance_Vec.%s", refdir, suf[k]);
    FILE *f = fopen(path, "wb");
    if (!f || (bytes[k] && fwrite(data[k], 1, bytes[k], f) != bytes[k]) || fclose(f) != 0) die("index_abv():%s", path);
  }
  mk_abv_destroy(a);
  free(ent); free(fend); free(names);
  return 0;
}
/* the result lines of one query, formatted by up to 16 threads into pieces that are then written in order */
typedef struct {
  const int32_t *ids;
  const float *m;
  char *const *names;
  uint64_t lo, hi;
  int l2;
  char *buf;
  size_t len;
} abv_fmt_job;
static void *abv_fmt_run(void *p) {
  abv_fmt_job *j = p;
  size_t cap = (size_t)(j->hi - j->lo) * 48 + 64;
  j->buf = malloc(cap);
  j->len = 0;
  for (uint64_t i = j->lo; i < j->hi && j->buf; i++) {
    const char *nm = j->names[j->ids[i]];
    const double v = j->l2 ? sqrt((double)j->m[i]) : (double)j->m[i]; /* :319 prints sqrt of the L2 sum */
    for (;;) {
      const int w = snprintf(j->buf + j->len, cap - j->len, "%s\t%lf\n", nm, v);
      if (w >= 0 && (size_t)w < cap - j->len) { j->len += (size_t)w; break; }
      cap = cap * 2 + (size_t)(w > 0 ? w : 64);
      char *nb = realloc(j->buf, cap);
      if (!nb) { free(j->buf); j->buf = NULL; break; }
      j->buf = nb;
    }
  }
  return NULL;
}
static void abv_print(const int32_t *ids, const float *m, uint64_t cnt, char *const *names, int l2) {
  abv_fmt_job jobs[16];
  int nt = (int)(cnt / 4096);
  if (nt < 1) nt = 1;
  if (nt > 16) nt = 16;
  pthread_t th[16];
  for (int t = 0; t < nt; t++) {
    jobs[t] = (abv_fmt_job){ids, m, names, cnt * (uint64_t)t / (uint64_t)nt, cnt * (uint64_t)(t + 1) / (uint64_t)nt, l2, NULL, 0};
    if (t && pthread_create(&th[t], NULL, abv_fmt_run, &jobs[t]) != 0) die("abv_search(): pthread_create");
  }
  abv_fmt_run(&jobs[0]);
  for (int t = 0; t < nt; t++) {
    if (t) pthread_join(th[t], NULL);
    if (!jobs[t].buf) die("abv_search(): out of memory");
    fwrite(jobs[t].buf, 1, jobs[t].len, stdout);
    free(jobs[t].buf);
  }
}
static int composite_search(const char *refdir, int metric, int nargs, char **args, int device) {
  char path[PATHLEN * 3 + 64];
  double t_read = 0, t_kernel = 0, t_fmt = 0, t0 = now_s();
  /* :218-252: names (fgets of PATHLEN, newline cut), norms, cumulative counts, matrix */
  size_t nn = 0, yn = 0, in = 0, mn = 0;
  snprintf(path, sizeof path, "%s/abundance_Vec.name", refdir);
  char *nb = (char *)read_whole(path, &nn);
  if (!nb) die("abv_search():%s", path);
  nb[nn] = 0;
  /* fgets(PATHLEN) pieces: up to PATHLEN - 1 bytes or through the newline; the name is the piece up to its newline */
  size_t ncap = 1024, S = 0, ol = 0;
  char **names = malloc(sizeof(char *) * ncap), *ob = malloc(2 * nn + 1);
  if (!names || !ob) die("abv_search(): out of memory");
  for (size_t pos = 0; pos < nn;) {
    size_t take = 0;
    while (take < PATHLEN - 1 && pos + take < nn) { if (nb[pos + take++] == '\n') break; }
    if (S == ncap) { ncap *= 2; names = realloc(names, sizeof(char *) * ncap); if (!names) die("abv_search(): out of memory"); }
    size_t l = strcspn(nb + pos, "\n");
    if (l > take) l = take;
    memcpy(ob + ol, nb + pos, l);
    ob[ol + l] = 0;
    names[S++] = ob + ol;
    ol += l + 1;
    pos += take;
  }
  if (S > 0xFFFFFFFFull) die("abv_search(): too many samples");
  snprintf(path, sizeof path, "%s/abundance_Vec.yl2n", refdir);
  double *yl2n = (double *)read_whole(path, &yn);
  if (!yl2n || yn < 8 * S) die("abv_search():%s", path);
  snprintf(path, sizeof path, "%s/abundance_Vec.abmi", refdir);
  int32_t *abmi = (int32_t *)read_whole(path, &in);
  if (!abmi) die("abv_search():%s", path);
  snprintf(path, sizeof path, "%s/abundance_Vec.abm", refdir);
  mk_binvec *abm = (mk_binvec *)read_whole(path, &mn);
  if (!abm) die("abv_search():%s", path);
  t_read += now_s() - t0;
  mk_abv *a = NULL; /* made (and the index loaded) at the first vector: arguments that are all skipped need no device */
  static const char *head[3] = {"CosineXY", "L1norm", "L2norm"};
  uint32_t batch = 64;
  if (S && (uint64_t)batch * S > 0xFFFFFFFFull) batch = (uint32_t)(0xFFFFFFFFull / S);
  if (batch < 1) batch = 1;
  int *qarg = malloc(sizeof(int) * (size_t)(nargs > 0 ? nargs : 1));
  uint64_t *qend = malloc(8 * (size_t)batch), *oend = malloc(8 * (size_t)batch);
  size_t qcap = 1 << 12;
  mk_binvec *qv = malloc(sizeof(mk_binvec) * qcap);
  for (int i = 0; i < nargs;) {
    /* a batch: arguments i .. j-1, of which nq are vectors; a file that cannot be read ends the batch before it */
    uint32_t nq = 0;
    uint64_t nd = 0;
    int j = i, fail = -1;
    t0 = now_s();
    for (; j < nargs && nq < batch; j++) {
      if (!abv_name_ok(args[j])) continue;
      if (strchr(args[j], '/')) snprintf(path, sizeof path, "%s", args[j]); /* :245-247 */
      else snprintf(path, sizeof path, "%s/abundance_Vec/%s", refdir, args[j]);
      FILE *f = fopen(path, "rb");
      struct stat fs;
      if (!f || fstat(fileno(f), &fs) != 0) { if (f) fclose(f); fail = j; break; }
      const uint64_t len = (uint64_t)fs.st_size / sizeof(mk_binvec);
      if (nd + len > qcap) { while (nd + len > qcap) qcap *= 2; qv = realloc(qv, sizeof(mk_binvec) * qcap); if (!qv) die("abv_search(): out of memory"); }
      if (len && fread(qv + nd, sizeof(mk_binvec), len, f) != len) { fclose(f); fail = j; break; }
      fclose(f);
      nd += len;
      qarg[nq] = j;
      qend[nq++] = nd;
    }
    t_read += now_s() - t0;
    const int32_t *ids = NULL;
    const float *ms = NULL;
    int64_t bad = -1;
    t0 = now_s();
    if (nq && !a) {
      if (mk_abv_create(device, &a) != MK_OK) die("mk_abv_create failed: %s", mk_abv_last_error(NULL));
      if (mk_abv_load(a, abm, mn / sizeof(mk_binvec), abmi, (uint32_t)(in / 4), yl2n, (uint32_t)S) != MK_OK)
        die("abv_search(): %s/abundance_Vec: %s", refdir, mk_abv_last_error(a));
    }
    if (nq && mk_abv_search(a, metric, nq, qv, qend, oend, &ids, &ms, &bad) != MK_OK) {
      if (bad >= 0) { /* the queries before the bad one are printed first, as the reference would have */
        nq = (uint32_t)bad;
        fail = -2;
        j = qarg[bad];
        if (nq && mk_abv_search(a, metric, nq, qv, qend, oend, &ids, &ms, NULL) != MK_OK) die("abv_search(): %s", mk_abv_last_error(a));
      } else die("abv_search(): %s", mk_abv_last_error(a));
    }
    t_kernel += now_s() - t0;
    t0 = now_s();
    uint32_t k = 0;
    for (; i < j; i++) {
      if (!abv_name_ok(args[i])) { printf("%dth argument %s is not a .abv file, skipped\n", i, args[i]); continue; }
      const uint64_t lo = k ? oend[k - 1] : 0, hi = oend[k];
      printf("#Sample\t%s\n", head[metric]);
      abv_print(ids + lo, ms + lo, hi - lo, names, metric == 2);
      k++;
    }
    t_fmt += now_s() - t0;
    if (fail == -2) {
      const char *p = args[j];
      die("abv_search(): %s: species outside the index", p);
    }
    if (fail >= 0) die("abv_search():%s: %s", path, strerror(errno ? errno : EIO));
  }
  if (a) mk_abv_destroy(a);
  fflush(stdout);
  if (getenv("MK_ABV_TIMES")) /* tools/bench_abv.py: where the command's wall time goes */
    fprintf(stderr, "{\"read_s\": %.6f, \"device_s\": %.6f, \"format_s\": %.6f}\n", t_read, t_kernel, t_fmt);
  free(qarg); free(qend); free(oend); free(qv); free(names); free(ob); free(nb); free(abm); free(abmi); free(yl2n);
  return 0;
}
/* one sample's rows, in print order, as the report line (command_composite.c:624) or as its .abv (:587-595, :615-636); the two float
 * divisions and the running float sum are the reference's, on the host */
void composite_write_sample(const mk_composite_row *rows, uint64_t nrows, const char *qname, const char *refname, const char *refdir,
                                   const char *outdir, int binvec, composite_vec *vec) {
  char path[PATHLEN * 3 + 64];
  FILE *vf = NULL;
  if (binvec) { /* :573-581 */
    char dir[PATHLEN * 2 + 32], qn[PATHLEN + 1];
    if (strlen(outdir) < 3) snprintf(dir, sizeof dir, "%s/abundance_Vec", refdir);
    else snprintf(dir, sizeof dir, "%s", outdir);
    mkdir(dir, 0777);
    snprintf(qn, sizeof qn, "%.*s", PATHLEN, qname);
    const char *base = strrchr(qn, '/');
    snprintf(path, sizeof path, "%s/%s.abv", dir, base ? base + 1 : qn);
    if (!(vf = fopen(path, "wb"))) die("get_species_abundance():%s", path);
  }
  int num_pass = 0;
  float vecsum = 0;
  for (uint64_t i = 0; i < nrows; i++) {
    const mk_composite_row *r = rows + i;
    if (binvec) {
      if (r->median > 1 && r->kmer_num > 7) {
        vec[num_pass].ref_idx = (int)r->ref;
        vec[num_pass].pct = (float)r->lastsum / r->lastn;
        vecsum += vec[num_pass].pct;
        num_pass++;
      }
    } else {
      printf("%.*s\t%.*s\t%d\t%f\t%f\t%d\t%d\n", PATHLEN, qname, PATHLEN, refname + (size_t)PATHLEN * r->ref, r->kmer_num,
             (float)r->sum / r->kmer_num, (float)r->lastsum / r->lastn, r->median, r->top);
    }
  }
  if (vf) {
    for (int i = 0; i < num_pass; i++) vec[i].pct = (vec[i].pct - 1) * 100 / (vecsum - num_pass);
    fwrite(vec, 8, (size_t)num_pass, vf);
    fclose(vf);
  }
}
/* bytes [off, off + len) of a file; die() with the reference's text when it cannot be had */
static void composite_read_range(const char *path, uint64_t off, void *dst, size_t len) {
  FILE *f = fopen(path, "rb");
  if (!f) die("get_species_abundance():%s", path);
  if (len && (fseeko(f, (off_t)off, SEEK_SET) != 0 || fread(dst, 1, len, f) != len)) die("get_species_abundance():%s is shorter than its index says", path);
  fclose(f);
}
/* `composite -r -q` with the marker database resident on the device (mk_composite): the database's components are read
 * and loaded once; the samples go through in batches of at most batch_bytes of query ids, of whose files only the batch's byte ranges
 * are read */
static void composite_resident(const char *refdir, const char *qrydir, const char *outdir, int binvec, int device, int ref_n, int qry_n,
                               int comp_num, const char *refname, const char *qryname, uint64_t batch_bytes, uint64_t *batches_out,
                               uint64_t *hits_out, double *load_ms, double *query_ms) {
  char path[PATHLEN * 3 + 64];
  mk_composite *h;
  if (mk_composite_create(device, &h) != MK_OK) die("mk_composite_create failed: %s", mk_composite_last_error(NULL));
  if (mk_composite_load_begin(h, (uint32_t)ref_n, (uint32_t)comp_num) != MK_OK) die("get_species_abundance(): %s", mk_composite_last_error(h));
  for (int c = 0; c < comp_num; c++) {
    size_t n1, n2;
    uint8_t *rco = need_part("get_species_abundance():", refdir, "combco", c, 0, &n1);
    uint8_t *ridx = need_part("get_species_abundance():", refdir, "combco.index", c, 8 * ((size_t)ref_n + 1), &n2);
    if (((const uint64_t *)ridx)[ref_n] * 4 > n1) die("get_species_abundance(): component %d is shorter than its index says", c);
    if (mk_composite_load_component(h, (uint32_t)c, (const uint32_t *)rco, (const uint64_t *)ridx) != MK_OK)
      die("get_species_abundance(): %s", mk_composite_last_error(h));
    free(rco); free(ridx);
  }
  /* the query's positions, every component */
  uint64_t **qpos = malloc(sizeof(uint64_t *) * (size_t)(comp_num > 0 ? comp_num : 1));
  for (int c = 0; c < comp_num; c++) {
    size_t n4;
    struct stat st;
    qpos[c] = (uint64_t *)need_part("get_species_abundance():", qrydir, "combco.index", c, 8 * ((size_t)qry_n + 1), &n4);
    snprintf(path, sizeof path, "%s/combco.%d", qrydir, c);
    if (stat(path, &st) != 0) die("get_species_abundance():%s", path);
    const uint64_t nid = (uint64_t)st.st_size;
    snprintf(path, sizeof path, "%s/combco.%d.a", qrydir, c);
    if (stat(path, &st) != 0) die("get_species_abundance():%s", path);
    if (qpos[c][qry_n] * 4 > nid || qpos[c][qry_n] * 2 > (uint64_t)st.st_size) die("get_species_abundance(): component %d is shorter than its index says", c);
    for (int q = 0; q < qry_n; q++)
      if (qpos[c][q] > qpos[c][q + 1]) die("get_species_abundance():%s/combco.index.%d does not ascend", qrydir, c);
  }
  composite_vec *vec = malloc(8 * ((size_t)ref_n + 1));
  uint64_t *local = malloc(8 * ((size_t)qry_n + 1)), *row_end = malloc(8 * ((size_t)qry_n + 1));
  uint32_t *ids = NULL;
  uint16_t *cnt = NULL;
  size_t cap = 0;
  uint64_t batches = 0, hits = 0;
  double qms = 0.0;
  for (int q0 = 0; q0 < qry_n;) {
    int q1 = q0;
    uint64_t bytes = 0;
    while (q1 < qry_n) { /* whole samples, at least one */
      uint64_t b = 0;
      for (int c = 0; c < comp_num; c++) b += (qpos[c][q1 + 1] - qpos[c][q1]) * 4;
      if (q1 > q0 && bytes + b > batch_bytes) break;
      bytes += b;
      q1++;
    }
    const int ns = q1 - q0;
    if (mk_composite_query_begin(h, (uint32_t)ns) != MK_OK) die("get_species_abundance(): %s", mk_composite_last_error(h));
    for (int c = 0; c < comp_num; c++) {
      const uint64_t a = qpos[c][q0], n = qpos[c][q1] - a;
      if (n > cap) {
        cap = n + n / 8 + 1024;
        free(ids); free(cnt);
        ids = malloc(4 * cap); cnt = malloc(2 * cap);
        if (!ids || !cnt) die("get_species_abundance(): out of memory");
      }
      snprintf(path, sizeof path, "%s/combco.%d", qrydir, c);
      composite_read_range(path, a * 4, ids, n * 4);
      snprintf(path, sizeof path, "%s/combco.%d.a", qrydir, c);
      composite_read_range(path, a * 2, cnt, n * 2);
      for (int k = 0; k <= ns; k++) local[k] = qpos[c][q0 + k] - a;
      if (mk_composite_query_component(h, (uint32_t)c, ids, cnt, local) != MK_OK) die("get_species_abundance(): %s", mk_composite_last_error(h));
    }
    const mk_composite_row *rows = NULL;
    if (mk_composite_query_finish(h, &rows, row_end) != MK_OK) die("get_species_abundance(): %s", mk_composite_last_error(h));
    for (int k = 0; k < ns; k++) {
      const uint64_t lo = k ? row_end[k - 1] : 0;
      composite_write_sample(rows + lo, row_end[k] - lo, qryname + (size_t)PATHLEN * (q0 + k), refname, refdir, outdir, binvec, vec);
    }
    uint64_t bh = 0, br = 0;
    double lm = 0.0, qm = 0.0;
    mk_composite_last_counts(h, &bh, &br);
    mk_composite_last_kernel_ms(h, &lm, &qm);
    hits += bh; qms += qm; *load_ms = lm;
    batches++;
    q0 = q1;
  }
  *batches_out = batches; *hits_out = hits; *query_ms = qms;
  mk_composite_destroy(h);
  for (int c = 0; c < comp_num; c++) free(qpos[c]);
  free(qpos); free(vec); free(local); free(row_end); free(ids); free(cnt);
}
int cmd_composite(int argc, char **argv) {
  const char *refdir = NULL, *qrydir = NULL, *outdir = "./";
  int binvec = 0, device = 0, route = 0 /* 1 --resident, 2 --per-query */, timing = 0;
  uint64_t batch_bytes = 256ull << 20; /* query ids of a batch on the resident route */
  for (int i = 0; i < argc; i++)
    if (!strcmp(argv[i], "-d")) { /* cmd_composite(): -d is looked at only without -r (command_composite.c:179-182) */
      int has_r = 0;
      for (int j = 0; j < argc; j++) has_r |= !strcmp(argv[j], "-r");
      if (!has_r) {
        char *files[4096];
        int nf = 0;
        for (int j = 0; j < argc && nf < 4096; j++)
          if (argv[j][0] != '-') files[nf++] = argv[j];
        if (nf < 1) { printf("\vUsage: kssd composite -d <query.abv>\n\v"); return 0; }
        return composite_read_abv(nf, files) == 1 ? 0 : 1;
      }
    }
  int index = 0, metric = -1, npos = 0;
  char **pos = NULL;
  for (int i = 0; i < argc; i++) {
    if (!strcmp(argv[i], "-r") && i + 1 < argc) refdir = argv[++i];
    else if (!strcmp(argv[i], "-q") && i + 1 < argc) qrydir = argv[++i];
    else if (!strcmp(argv[i], "-o") && i + 1 < argc) outdir = argv[++i];
    else if (!strcmp(argv[i], "-p") && i + 1 < argc) ++i;
    else if (!strcmp(argv[i], "-b")) binvec = 1;
    else if (!strcmp(argv[i], "-i")) index = 1;
    else if (!strcmp(argv[i], "-s") && i + 1 < argc) metric = atoi(argv[++i]); /* :83: atoi, as argp hands it over */
    else if (!strncmp(argv[i], "-s", 2) && argv[i][2] && argv[i][2] != '-') metric = atoi(argv[i] + 2); /* -s1, the README's form */
    else if (!strcmp(argv[i], "--device") && i + 1 < argc) device = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--resident")) route = 1;
    else if (!strcmp(argv[i], "--per-query")) route = 2;
    else if (!strcmp(argv[i], "--timing")) timing = 1;
    else if (!strcmp(argv[i], "--batch-mib") && i + 1 < argc) batch_bytes = strtoull(argv[++i], NULL, 10) << 20; /* test hook: 0 = a sample a batch */
    else if (argv[i][0] != '-') { pos = argv + i; npos = argc - i; break; } /* ARGP_KEY_ARGS: the rest are the query vectors */
    else die("composite option %s is not part of this build (-r -q -i -s -b -o and -d are)", argv[i]);
  }
  /* cmd_composite() :170-178: -q, else -i, else -s, else the usage line */
  if (refdir && !qrydir) {
    if (index) return composite_index(refdir, device);
    if (metric != -1) {
      if (metric >= 0 && metric < 3 && npos > 0) return composite_search(refdir, metric, npos, pos, device);
      printf("\vUsage: metakssd composite -r <ref> -s <0|1|2> <query.abv>\n\v");
      return 0;
    }
    printf("\vUsage: metakssd composite -r <ref> < mode: -q | -i | -s >\n\v");
    return 0;
  }
  if (!refdir || !qrydir || !strcmp(refdir, qrydir)) die("get_species_abundance(): refdir or qrydir is not initialized");
  char path[PATHLEN * 3 + 64];
  costat rs, qs;
  const int rhave = costat_load(refdir, &rs);
  if (rhave == COSTAT_ABSENT) die("cannot find cofiles.stat under %s ", refdir);
  const int qhave = costat_load(qrydir, &qs);
  if (qhave == COSTAT_ABSENT) die("cannot find cofiles.stat under %s ", qrydir);
  const int32_t ref_n = rs.infile_num, qry_n = qs.infile_num, comp_num = rs.comp_num;
  if (!qs.koc) die("get_species_abundance(): query has not abundance");
  if (qs.shuf_id != rs.shuf_id) printf("get_species_abundance(): qry shuf_id %u not match ref shuf_id: %u\n", qs.shuf_id, rs.shuf_id);
  if (rhave < COSTAT_FULL || qhave < COSTAT_FULL) die("get_species_abundance(): truncated cofiles.stat");
  const char *refname = rs.names, *qryname = qs.names;

  /* two routes to the same bytes: the marker database resident on the device and the samples in batches -- the default
   * from two samples on -- or the reference's loop, one join per sample and component (one sample: strictly less work) */
  if (route == 1 || (route == 0 && qry_n >= 2)) {
    uint64_t batches = 0, hits = 0;
    double load_ms = 0.0, query_ms = 0.0;
    composite_resident(refdir, qrydir, outdir, binvec, device, ref_n, qry_n, comp_num, refname, qryname, batch_bytes, &batches, &hits, &load_ms, &query_ms);
    if (timing)
      printf("{\"composite_timing\": {\"route\": \"resident\", \"samples\": %d, \"batches\": %llu, \"hits\": %llu, \"load_kernel_ms\": %.3f, \"query_kernel_ms\": %.3f}}\n",
             qry_n, (unsigned long long)batches, (unsigned long long)hits, load_ms, query_ms);
    free(rs.raw); free(qs.raw);
    return 0;
  }
  mk_setop *so;
  if (mk_setop_create(device, &so) != MK_OK) die("mk_setop_create failed: %s", mk_setop_last_error(NULL));
  uint64_t pq_hits = 0;
  double pq_join_ms = 0.0;
  mk_composite_row *prow = malloc(sizeof(mk_composite_row) * ((size_t)ref_n + 1));
  int **vals = calloc((size_t)ref_n, sizeof(int *)); /* per reference sketch: the query's counts of the shared k-mers */
  int *nval = calloc((size_t)ref_n, sizeof(int)), *cap = calloc((size_t)ref_n, sizeof(int));
  uint64_t *seg = malloc(8 * ((size_t)ref_n + 1));
  int *order = malloc(sizeof(int) * (size_t)ref_n), *tmp = malloc(sizeof(int) * (size_t)ref_n);
  composite_vec *vec = malloc(8 * ((size_t)ref_n + 1));

  for (int q = 0; q < qry_n; q++) {
    for (int r = 0; r < ref_n; r++) nval[r] = 0;
    for (int c = 0; c < comp_num; c++) {
      size_t n1, n2, n3, n4, n5;
      uint8_t *rco = need_part("get_species_abundance():", refdir, "combco", c, 0, &n1);
      uint8_t *ridx = need_part("get_species_abundance():", refdir, "combco.index", c, 8 * ((size_t)ref_n + 1), &n2);
      uint8_t *qco = need_part("get_species_abundance():", qrydir, "combco", c, 0, &n3);
      uint8_t *qidx = need_part("get_species_abundance():", qrydir, "combco.index", c, 8 * ((size_t)qry_n + 1), &n4);
      snprintf(path, sizeof path, "%s/combco.%d.a", qrydir, c);
      uint8_t *qab = read_whole(path, &n5);
      if (!qab) die("get_species_abundance():%s", path);
      const uint64_t *rpos = (const uint64_t *)ridx, *qpos = (const uint64_t *)qidx;
      if (rpos[ref_n] * 4 > n1 || qpos[qry_n] * 4 > n3 || qpos[qry_n] * 2 > n5) die("get_species_abundance(): component %d is shorter than its index says", c);
      const uint32_t *counts = NULL;
      uint64_t m = 0;
      if (mk_setop_join(so, (const uint32_t *)qco + qpos[q], (const uint16_t *)qab + qpos[q], qpos[q + 1] - qpos[q], (const uint32_t *)rco,
                        rpos[ref_n], rpos, (uint32_t)ref_n + 1, &counts, &m, seg) != MK_OK)
        die("get_species_abundance(): %s", mk_setop_last_error(so));
      if (timing) { double ms = 0.0; mk_setop_last_join_ms(so, &ms); pq_join_ms += ms; pq_hits += m; }
      for (int r = 0; r < ref_n; r++) {
        const int k = (int)(seg[r + 1] - seg[r]);
        if (nval[r] + k > cap[r]) {
          cap[r] = (nval[r] + k) * 2 + 8;
          vals[r] = realloc(vals[r], sizeof(int) * (size_t)cap[r]);
        }
        for (int j = 0; j < k; j++) vals[r][nval[r] + j] = (int)counts[seg[r] + (uint64_t)j];
        nval[r] += k;
      }
      free(rco); free(ridx); free(qco); free(qidx); free(qab);
    }
    /* references by decreasing number of shared k-mers; ties keep their index order (what glibc's merge-sort qsort gives
     * the reference, :568-570): bottom-up merge sort */
    for (int i = 0; i < ref_n; i++) order[i] = i;
    for (int w = 1; w < ref_n; w *= 2) {
      for (int lo = 0; lo < ref_n; lo += 2 * w) {
        const int mid = lo + w < ref_n ? lo + w : ref_n, hi = lo + 2 * w < ref_n ? lo + 2 * w : ref_n;
        int a = lo, b = mid, k = lo;
        while (a < mid && b < hi) tmp[k++] = nval[order[b]] > nval[order[a]] ? order[b++] : order[a++];
        while (a < mid) tmp[k++] = order[a++];
        while (b < hi) tmp[k++] = order[b++];
      }
      memcpy(order, tmp, sizeof(int) * (size_t)ref_n);
    }
    uint64_t nrows = 0;
    for (int i = 0; i < ref_n; i++) {
      const int r = order[i], kmer_num = nval[r];
      if (kmer_num < 6) break; /* MIN_KM_S */
      int *v = vals[r] - 1;    /* 1-based like the reference's ref_abund[r][1..kmer_num] */
      qsort(vals[r], (size_t)kmer_num, sizeof(int), cmp_int_asc);
      int sum = 0;
      for (int n = 1; n <= kmer_num; n++) sum += v[n];
      const int median_idx = kmer_num / 2, pct_idx = kmer_num * 0.98; /* ST_PCTL */
      int lastsum = 0, lastn = 0;
      for (int n = pct_idx; n <= kmer_num * 0.99; n++) { lastsum += v[n]; lastn++; } /* ED_PCTL */
      prow[nrows++] = (mk_composite_row){(uint32_t)r, kmer_num, sum, lastsum, lastn, v[median_idx], v[kmer_num]};
    }
    composite_write_sample(prow, nrows, qryname + (size_t)PATHLEN * q, refname, refdir, outdir, binvec, vec);
  }
  if (timing)
    printf("{\"composite_timing\": {\"route\": \"per-query\", \"samples\": %d, \"batches\": %d, \"hits\": %llu, \"load_kernel_ms\": 0.000, \"query_kernel_ms\": %.3f}}\n",
           qry_n, qry_n, (unsigned long long)pq_hits, pq_join_ms);
  free(prow);
  mk_setop_destroy(so);
  for (int r = 0; r < ref_n; r++) free(vals[r]);
  free(vals); free(nval); free(cap); free(seg); free(order); free(tmp); free(vec); free(rs.raw); free(qs.raw);
  return 0;
}
