/* cli_db.c -- the database side of `dist`: stage II (`dist -o <mco> <sketch dir>`), the directory combiner, the search
 * (`dist -r <mco> <sketch dir>`), and `shuffle` */
#include "cli.h"

/* run_stageII() + combco2mco() (command_dist.c:504-552, co2mco.c:12-87): mcofiles.stat, mco.N, mco.index.N */
int run_stage2(const char *codir, const char *mcodir, int device, int quiet) {
  char path[PATHLEN * 2 + 32];
  costat s;
  if (costat_load(codir, &s) < COSTAT_FULL) die("run_stageII(():%s", s.path);
  const int32_t comp_num = s.comp_num, cofnum = s.infile_num;
  if (mkdir(mcodir, 0700)) {
    if (errno == EEXIST) printf("Warning: write mco file to an exists outdir:%s\n", mcodir);
    else die("run_stageII(): mkdir %s error", mcodir);
  }
  snprintf(path, sizeof path, "%s/mcofiles.stat", mcodir);
  FILE *f = fopen(path, "wb");
  if (!f) die("run_stageII(():%s", path);
  const int32_t mh[5] = {(int32_t)s.shuf_id, s.kmerlen, s.dim_rd_len, s.comp_num, s.infile_num};
  fwrite(mh, 4, 5, f);                                      /* mco_dstat_t (command_dist.h:66-75) */
  fwrite(s.ctx_ct, 1, (size_t)cofnum * (4 + PATHLEN), f); /* per-sketch k-mer counts, names */
  if (fclose(f)) die("run_stageII(():%s", path);
  mk_mco *m;
  if (mk_mco_create(device, &m) != MK_OK) die("mk_mco_create failed: %s", mk_mco_last_error(NULL));
  const uint64_t slab = 1ull << 27;
  uint64_t *rows = NULL; /* pinned: the slabs come back at PCIe speed instead of through a pageable bounce buffer */
  if (mk_host_alloc((void **)&rows, slab * 8) != MK_OK) die("out of memory");
  for (int c = 0; c < comp_num; c++) {
    size_t nb = 0, ib = 0;
    uint8_t *idx = need_part("", codir, "combco.index", c, 8 * ((size_t)cofnum + 1), &ib);
    uint8_t *ids = read_part(path, sizeof path, codir, "combco", c, 0, &nb);
    if (!ids || nb / 4 < ((const uint64_t *)idx)[cofnum]) die("%s", path);
    const uint32_t *gids, *row_ids;
    const uint64_t *row_ends;
    uint64_t n, nrows;
    int rc = mk_mco_build(m, (const uint32_t *)ids, (const uint64_t *)idx, (uint32_t)cofnum, &gids, &n, &row_ids, &row_ends, &nrows);
    if (rc != MK_OK) die("mk_mco_build failed (%d): %s", rc, mk_mco_last_error(m));
    free(ids); free(idx);
    snprintf(path, sizeof path, "%s/mco.index.%d", mcodir, c);
    f = fopen(path, "wb");
    if (!f) die("%s", path);
    const uint64_t comp_rows = 1ull << (4 * g_opt.component_sz); /* 1LLU << 4*COMPONENT_SZ rows, co2mco.c:19, 63-66 */
    for (uint64_t r0 = 0; r0 < comp_rows; r0 += slab) {
      const uint64_t nr = comp_rows - r0 < slab ? comp_rows - r0 : slab;
      rc = mk_mco_index_rows(m, r0, nr, rows);
      if (rc != MK_OK) die("mk_mco_index_rows failed (%d): %s", rc, mk_mco_last_error(m));
      if (fwrite(rows, 8, nr, f) != nr) die("%s: write failed", path);
    }
    if (fclose(f)) die("%s: write failed", path);
    snprintf(path, sizeof path, "%s/mco.%d", mcodir, c);
    f = fopen(path, "wb");
    if (!f) die("combco2mco()::%s", path);
    if (n && fwrite(gids, 4, n, f) != n) die("%s: write failed", path);
    if (fclose(f)) die("%s: write failed", path);
    if (!quiet) printf("component %d: %llu ids in %llu rows\n", c, (unsigned long long)n, (unsigned long long)nrows);
  }
  mk_host_free(rows); free(s.raw);
  mk_mco_destroy(m);
  return 0;
}
/* combine_queries() (command_dist.c:1718-1924): `dist -o <out> <sketch dir> <sketch dir>...` strings several sketch directories
 * (batches of queries) together: combco.N appended, combco.index.N continued with the running offset, the cofiles.stat
 * header of the first directory with the summed sketch and k-mer counts, then everybody's count lists and names.  Host only.
 * As there: -A sketches are refused, a directory without cofiles.stat, with another shuf_id or with abundances is skipped
 * with a message. */
int run_combine(int ndirs, char **dirs, const char *outdir) {
  char path[PATHLEN * 2 + 32];
  mkdir(outdir, 0700);
  costat s0;
  const int have0 = costat_load(dirs[0], &s0);
  if (have0 == COSTAT_ABSENT) die("combine_queries():%s", s0.path);
  if (s0.koc) die("combine_queries(): abundance model not supported yet");
  const uint32_t id0 = s0.shuf_id;
  const int32_t comp_num = s0.comp_num;
  int32_t infile_num = s0.infile_num;
  uint64_t all_ctx_ct = s0.all_ctx_ct;
  if (have0 < COSTAT_FULL) die("combine_queries():%s", s0.path);
  /* count lists and name records of every accepted directory, in order */
  size_t ct_bytes = 0, nm_bytes = 0;
  uint8_t *cts = NULL, *nms = NULL;
#define APPEND(buf, len, src, n) do { buf = realloc(buf, len + (n)); if (!buf) die("out of memory"); memcpy(buf + len, src, n); len += (n); } while (0)
  APPEND(cts, ct_bytes, s0.ctx_ct, 4 * (size_t)infile_num);
  APPEND(nms, nm_bytes, s0.names, (size_t)PATHLEN * infile_num);
  FILE **co = malloc(sizeof(FILE *) * (size_t)comp_num), **ix = malloc(sizeof(FILE *) * (size_t)comp_num);
  uint64_t *offset = calloc((size_t)comp_num, 8);
  for (int c = 0; c < comp_num; c++) {
    size_t nb = 0, ib = 0;
    snprintf(path, sizeof path, "%s/combco.%d", outdir, c);
    if (!(co[c] = fopen(path, "wb"))) die("%s", path);
    snprintf(path, sizeof path, "%s/combco.index.%d", outdir, c);
    if (!(ix[c] = fopen(path, "wb"))) die("%s", path);
    uint8_t *ids = read_part(path, sizeof path, dirs[0], "combco", c, 0, &nb);
    if (!ids) die("%s", path);
    if (nb && fwrite(ids, 1, nb, co[c]) != nb) die("%s: write failed", path);
    free(ids);
    uint8_t *idx = read_part(path, sizeof path, dirs[0], "combco.index", c, 8, &ib);
    if (!idx) die("%s", path);
    if (fwrite(idx, 1, ib, ix[c]) != ib) die("%s: write failed", path);
    memcpy(&offset[c], idx + ib - 8, 8);
    free(idx);
  }
  for (int i = 1; i < ndirs; i++) {
    costat si;
    const int have = costat_load(dirs[i], &si);
    const int32_t fi = si.infile_num;
    if (have == COSTAT_ABSENT) { printf("%dth query %s is not a valid query: no %s file\n", i, dirs[i], "cofiles.stat"); free(si.raw); continue; }
    if (si.shuf_id != id0) { printf("combine_queries(): %dth shuf_id: %u not match 0th shuf_id: %u\n", i, si.shuf_id, id0); free(si.raw); continue; }
    if (si.koc) { printf("combine_queries(): %dth query abundance model not supported yet \n", i); free(si.raw); continue; }
    if (have < COSTAT_FULL) die("combine_queries():%s", si.path);
    all_ctx_ct += si.all_ctx_ct;
    infile_num += fi;
    APPEND(cts, ct_bytes, si.ctx_ct, 4 * (size_t)fi);
    APPEND(nms, nm_bytes, si.names, (size_t)PATHLEN * fi);
    free(si.raw);
    for (int c = 0; c < comp_num; c++) {
      size_t nb = 0, ib = 0;
      uint8_t *ids = read_part(path, sizeof path, dirs[i], "combco", c, 0, &nb);
      if (!ids) die("%s", path);
      if (nb && fwrite(ids, 1, nb, co[c]) != nb) die("%s: write failed", path);
      free(ids);
      uint64_t *idx = (uint64_t *)read_part(path, sizeof path, dirs[i], "combco.index", c, 8, &ib);
      if (!idx) die("%s", path);
      const size_t ne = ib / 8;
      for (size_t k = 1; k < ne; k++) idx[k] += offset[c];
      if (ne > 1 && fwrite(idx + 1, 8, ne - 1, ix[c]) != ne - 1) die("%s: write failed", path);
      offset[c] = idx[ne - 1];
      free(idx);
    }
  }
#undef APPEND
  for (int c = 0; c < comp_num; c++)
    if (fclose(co[c]) || fclose(ix[c])) die("combine_queries(): write failed");
  costat_set_totals(&s0, infile_num, s0.koc, all_ctx_ct);
  snprintf(path, sizeof path, "%s/cofiles.stat", outdir);
  FILE *f = fopen(path, "wb");
  if (!f || fwrite(s0.raw, 1, s0.hdr, f) != s0.hdr || fwrite(cts, 1, ct_bytes, f) != ct_bytes || fwrite(nms, 1, nm_bytes, f) != nm_bytes || fclose(f))
    die("%s: write failed", path);
  free(s0.raw); free(cts); free(nms); free(co); free(ix); free(offset);
  return 0;
}
typedef struct {
  const uint64_t *index;
  const uint32_t *ids;
  uint64_t *es, *ee;
  uint64_t lo, hi;
} extent_job;
static void *extent_worker(void *arg) { /* command_dist.c:1040-1041: the row of k-mer id `ind` in the mmap'ed index */
  extent_job *j = arg;
  for (uint64_t i = j->lo; i < j->hi; i++) {
    const uint32_t ind = j->ids[i];
    j->es[i] = ind > 0 ? j->index[ind - 1] : 0;
    j->ee[i] = j->index[ind];
  }
  return NULL;
}
/* mco_cbdco_nobin_dist() (command_dist.c:902-1079): `dist -r <mco dir> -o <outdir> <sketch dir>` */
int run_search(const char *refdir, const char *qrydir, const char *outdir, const mk_dist_opts *o, int keep_shared, const char *skf,
               int device, int nthreads, int quiet) {
  char path[PATHLEN * 2 + 32];
  mkdir(outdir, 0700);
  costat rs, qs;
  const int rhave = mcostat_load(refdir, &rs);
  if (rhave == COSTAT_ABSENT) die("need provied mco dir path for mco_co_dist() arg 1. refmco_dstat_fpath");
  const int qhave = costat_load(qrydir, &qs);
  if (qhave == COSTAT_ABSENT) die("need provied co dir path for mco_co_dist() arg 2.  qryco_dstat_fpath");
  const int32_t r_comp = rs.comp_num, ref_num = rs.infile_num, q_k = qs.kmerlen, q_dr = qs.dim_rd_len, qry_num = qs.infile_num;
  if (qs.shuf_id != rs.shuf_id) die("qry shuf_id: %d not match ref shuf_id: %d\ntry regenerate .co dir and feed -s the .shuffile used to generated ref database", qs.shuf_id, rs.shuf_id);
  if (qs.comp_num != r_comp) die("qry comp_num: %d not match ref comp_num: %d", qs.comp_num, r_comp);
  if (rhave < COSTAT_FULL || qhave < COSTAT_FULL) die("truncated stat file under %s or %s", refdir, qrydir);
  const uint32_t *ref_ct = rs.ctx_ct, *qry_ct = qs.ctx_ct;
  const char *refnames = rs.names, *qrynames = qs.names;
  const size_t cells = (size_t)ref_num * (size_t)qry_num;
  char skpath[PATHLEN * 2 + 32];
  snprintf(skpath, sizeof skpath, "%s/sharedk_ct.dat", outdir);
  uint32_t *ct = NULL;
  if (skf && skf[0]) { /* -f: print from an earlier run's counts (:987-990) */
    size_t sb = 0;
    snprintf(skpath, sizeof skpath, "%s", skf);
    ct = (uint32_t *)read_whole(skpath, &sb);
    if (!ct || sb < cells * 4) die("open %s failed", skpath);
  } else {
    FILE *probe = fopen(skpath, "rb");
    if (probe) { fclose(probe); die(" mco_cbdco_nobin_dist():%s: File exists", skpath); } /* :954-960 */
    ct = calloc(cells + 1, 4);
    if (!ct) die("out of memory");
    if (!quiet) printf("disf_sz=%lu\trefnum=%d\tqrynum=%d\tnum_mapping_distf=%d\tbatch_qrynum=%d\t%lu\t%lu\n", (unsigned long)(cells * 4), ref_num,
                       qry_num, 0, qry_num, (unsigned long)(cells * 4), 0ul);
    mk_mco *m;
    if (mk_mco_create(device, &m) != MK_OK) die("mk_mco_create failed: %s", mk_mco_last_error(NULL));
    int rc = mk_mco_count_begin(m, (uint32_t)ref_num, (uint32_t)qry_num);
    if (rc != MK_OK) die("mk_mco_count_begin failed (%d): %s", rc, mk_mco_last_error(m));
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 24) nthreads = 24; /* 20-24 framer threads keep PCIe busy; more only take memory bandwidth from the copies */
    for (int c = 0; c < r_comp; c++) {
      size_t gb = 0, xb = 0, ib = 0, cb = 0;
      snprintf(path, sizeof path, "%s/mco.index.%d", refdir, c);
      const uint64_t *index = map_whole(path, &xb);
      if (!index || xb != (8ull << (4 * g_opt.component_sz))) die("%s: not a 16^%d-row index (--component-sz)", path, g_opt.component_sz);
      snprintf(path, sizeof path, "%s/mco.%d", refdir, c);
      const uint32_t *gids = map_whole(path, &gb);
      if (!gids && gb) die("%s", path);
      uint8_t *qidx = need_part("", qrydir, "combco.index", c, 8 * ((size_t)qry_num + 1), &ib);
      uint8_t *qids = read_part(path, sizeof path, qrydir, "combco", c, 0, &cb);
      const uint64_t nq = ((const uint64_t *)qidx)[qry_num];
      if (!qids || cb / 4 < nq) die("%s", path);
      uint64_t *es = malloc(8 * (nq + 1)), *ee = malloc(8 * (nq + 1));
      if (!es || !ee) die("out of memory");
      pthread_t th[64];
      extent_job jobs[64];
      int started = 0;
      for (int t = 0; t < nthreads; t++) {
        jobs[t] = (extent_job){index, (const uint32_t *)qids, es, ee, nq * (uint64_t)t / (uint64_t)nthreads, nq * (uint64_t)(t + 1) / (uint64_t)nthreads};
        if (t + 1 == nthreads || pthread_create(&th[started], NULL, extent_worker, &jobs[t]) != 0) extent_worker(&jobs[t]);
        else started++;
      }
      for (int t = 0; t < started; t++) pthread_join(th[t], NULL);
      static const uint32_t no_gids = 0; /* a database of empty sketches has an empty mco.N: still a valid (all-zero) search */
      rc = mk_mco_count_add(m, gids ? gids : &no_gids, gb / 4, NULL, es, ee, (const uint64_t *)qidx, qry_ct);
      if (rc != MK_OK) die("mk_mco_count_add failed (%d): %s", rc, mk_mco_last_error(m));
      free(es); free(ee); free(qids); free(qidx);
      munmap((void *)index, xb);
      if (gids) munmap((void *)gids, gb);
    }
    rc = mk_mco_count_finish(m, ct);
    if (rc != MK_OK) die("mk_mco_count_finish failed (%d): %s", rc, mk_mco_last_error(m));
    mk_mco_destroy(m);
    FILE *sk = fopen(skpath, "wb");
    if (!sk) die(" mco_cbdco_nobin_dist()::%s", skpath);
    if (cells && fwrite(ct, 4, cells, sk) != cells) die("%s: write failed", skpath);
    if (fclose(sk)) die("%s: write failed", skpath);
  }
  snprintf(path, sizeof path, "%s/distance.out", outdir);
  FILE *fp = fopen(path, "w");
  if (!fp) die("dist_print_nobin():%s", path);
  if (o->num_neigb > 1024 || o->num_neigb > ref_num) die("neighborN_max %d should smaller than NREF %d and ref_num %d", o->num_neigb, 1024, ref_num);
  int rc = mk_dist_print(fp, o, q_k, q_dr, (uint32_t)ref_num, (uint32_t)qry_num, ref_ct, qry_ct, refnames, qrynames, ct);
  if (rc != MK_OK) die("mk_dist_print failed (%d)", rc);
  if (fclose(fp)) die("%s: write failed", path);
  if (!keep_shared) remove(skpath); /* :1633 (also a file given with -f) */
  free(ct); free(rs.raw); free(qs.raw);
  return 0;
}
int cmd_shuffle(int argc, char **argv) {
  int k = 8, s = 5, l = 2;
  unsigned long long seed = 1;
  const char *out = "default";
  for (int i = 0; i < argc; i++) {
    if (!strcmp(argv[i], "-k") && i + 1 < argc) k = atoi(argv[++i]);
    else if (!strcmp(argv[i], "-s") && i + 1 < argc) s = atoi(argv[++i]);
    else if (!strcmp(argv[i], "-l") && i + 1 < argc) l = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--seed") && i + 1 < argc) seed = strtoull(argv[++i], NULL, 10);
    else if (!strcmp(argv[i], "-o") && i + 1 < argc) out = argv[++i];
    else usage();
  }
  mk_shuf sh;
  if (mk_shuf_generate(k, s, l, seed, &sh) != MK_OK) die("shuffle: invalid -k/-s/-l (need subk <= k, subk < 8: command_shuffle.c:176-181)");
  char path[PATHLEN * 2];
  snprintf(path, sizeof path, "%s.shuf", out);
  if (mk_shuf_write(&sh, path) != MK_OK) die("write_dim_shuffle_file(): open file %s failed", path);
  printf("kssd shuffle: shuf_id=%d, k = %d, halfCtxLen = %d, level= %d\n", sh.id, sh.k, sh.subk, sh.drlevel);
  mk_shuf_free(&sh);
  return 0;
}
