/* cli_set.c -- `metakssd set`: -u / -q / -i / -s / -g / -c / -P (command_set.c) */
#include "cli.h"

/* `set -P`: print_gnames(), command_set.c:610-631 */
static int set_print_names(const char *in) {
  costat s;
  const int have = costat_load(in, &s);
  if (have == COSTAT_ABSENT) die("cannot find cofiles.stat under %s ", in);
  if (have < COSTAT_FULL) die("sketch_union():%s", s.path);
  for (int i = 0; i < s.infile_num; i++) printf("%d\t%.*s\n", (int)s.ctx_ct[i], PATHLEN, s.names + (size_t)PATHLEN * i);
  free(s.raw);
  return 0;
}
/* `set -i <pan>` / `set -s <pan>`: sketch_operate(), command_set.c:321-425.  Dictionary of the pan ids and the ordered
 * filter on the device (mk_setop_filter); files, per-file recount and the untouched header fields as in the reference. */
static int set_operate(const char *in, const char *pan, const char *outdir, int intersect, int device) {
  char path[PATHLEN * 2 + 32];
  costat ps, s;
  if (costat_load(pan, &ps) == COSTAT_ABSENT) die("cannot find cofiles.stat under %s ", pan);
  const int have = costat_load(in, &s);
  if (have == COSTAT_ABSENT) die("cannot find cofiles.stat under %s ", in);
  const int32_t pan_comp = ps.comp_num, infile_num = s.infile_num;
  free(ps.raw);
  if (ps.shuf_id != s.shuf_id) die("sketcing id not match(%d Vs. %d)", (int)s.shuf_id, (int)ps.shuf_id);
  if (have < COSTAT_COUNTS) die("sketch_operate():%s", s.path);
  uint32_t *ctx_ct = s.ctx_ct;
  memset(ctx_ct, 0, 4 * (size_t)infile_num); /* :344-345: recounted below; all_ctx_ct stays as it was */
  mkdir(outdir, 0777);
  mk_setop *so;
  if (mk_setop_create(device, &so) != MK_OK) die("mk_setop_create failed: %s", mk_setop_last_error(NULL));
  uint64_t *post = malloc(8 * ((size_t)infile_num + 1));
  for (int c = 0; c < pan_comp; c++) {
    size_t nb = 0, ib = 0, cb = 0;
    uint8_t *pids = read_part(path, sizeof path, pan, "pan", c, 0, &nb);
    if (!pids) pids = read_part(path, sizeof path, pan, "uniq_pan", c, 0, &nb); /* :369-372 */
    if (!pids) die("sketch_operate():%s", path);
    uint8_t *idx = need_part("sketch_operate():", in, "combco.index", c, 8 * ((size_t)infile_num + 1), &ib);
    uint8_t *co = need_part("sketch_operate():", in, "combco", c, 0, &cb);
    const uint64_t *pos = (const uint64_t *)idx;
    const uint64_t n = pos[infile_num];
    if (n * 4 > cb) die("sketch_operate():%s/combco.%d is shorter than its index says", in, c);
    const uint32_t *out = NULL;
    uint64_t m = 0;
    if (mk_setop_begin(so, MK_SET_UNION) != MK_OK || mk_setop_add(so, (const uint32_t *)pids, nb / 4) != MK_OK ||
        mk_setop_filter(so, intersect, (const uint32_t *)co, n, pos, (uint32_t)infile_num + 1, &out, &m, post) != MK_OK)
      die("sketch_operate(): %s", mk_setop_last_error(so));
    for (int i = 0; i < infile_num; i++) ctx_ct[i] += (uint32_t)(post[i + 1] - post[i]);
    FILE *f;
    snprintf(path, sizeof path, "%s/combco.%d", outdir, c);
    if (!(f = fopen(path, "wb")) || fwrite(out, 4, m, f) != m) die("sketch_operate():%s", path);
    fclose(f);
    snprintf(path, sizeof path, "%s/combco.index.%d", outdir, c);
    if (!(f = fopen(path, "wb")) || fwrite(post, 8, (size_t)infile_num + 1, f) != (size_t)infile_num + 1) die("sketch_operate():%s", path);
    fclose(f);
    free(pids); free(idx); free(co);
  }
  free(post);
  mk_setop_destroy(so);
  snprintf(path, sizeof path, "%s/cofiles.stat", outdir);
  FILE *f = fopen(path, "wb");
  if (!f || fwrite(s.raw, 1, s.n, f) != s.n) die("sketch_operate():%s", path);
  fclose(f);
  free(s.raw);
  return 0;
}
/* `set -g <file.tsv>`: grouping_genomes() (command_set.c:831-974) on top of organize_taxf() (:635-705).
 * Line i of the category file ("<taxid>[TAB<name>]") classifies sketch i.  The taxa are visited in the slot order of the
 * reference's hash of taxids (table of nextPrime(lines / 0.6) slots, double hashing) -- that order is part of the output.
 * Per taxon and component the concatenated id lists of its sketches go through mk_setop_group. */
typedef struct { int taxid; char *name; int *gids; int ng; } taxon_t;

static int next_prime_from(int n) { /* global_basic.c:453-475 */
  for (;; n++) {
    int composite = 0;
    for (int j = 2; (long long)j * j <= n; j++)
      if (n % j == 0) { composite = 1; break; }
    if (!composite) return n;
  }
}
static int set_group(const char *in, const char *taxfile, const char *outdir, int device) {
  size_t tn = 0;
  uint8_t *txt = read_whole(taxfile, &tn);
  if (!txt) die("%s: %s", taxfile, strerror(errno));
  int nlines = 0;
  for (size_t i = 0; i < tn; i++) nlines += txt[i] == '\n';
  const int tsz = next_prime_from((int)((double)nlines / 0.6)); /* LD_FCTR */
  taxon_t *slots = calloc((size_t)tsz, sizeof *slots);
  for (int i = 0; i < tsz; i++) slots[i].taxid = -1;
  int ntax = 0;
  size_t at = 0;
  for (int i = 0; i < nlines; i++) {
    size_t e = at;
    while (txt[e] != '\n') e++;
    if (e - at + 1 >= PATHLEN) die("organize_taxf(): %dth line %.40s is not full read, exceed PATHLEN %d ", i, (char *)txt + at, PATHLEN);
    txt[e] = 0;
    char *save = NULL;
    char *tok = strtok_r((char *)txt + at, "\t", &save);
    at = e + 1;
    if (!tok) die("organize_taxf(): %dth line of %s is empty", i, taxfile);
    const int taxid = atoi(tok);
    const char *name = strtok_r(NULL, "\t", &save);
    if (taxid < 0) die("organize_taxf(): negative taxid %d in %dth line", taxid, i);
    for (int n = 0; n < tsz; n++) {
      const int hv = (taxid % tsz + n * (1 + taxid % (tsz - 1))) % tsz;
      if (hv < 0) die("organize_taxf(): taxid %d overflows the category hash", taxid);
      taxon_t *t = &slots[hv];
      if (t->taxid == -1) {
        t->taxid = taxid; t->name = name ? strdup(name) : NULL;
        t->gids = malloc(sizeof(int)); t->gids[0] = i; t->ng = 1;
        ntax++;
        break;
      }
      if (t->taxid == taxid) {
        if ((t->name == NULL) != (name == NULL) || (name && strcmp(t->name, name) != 0))
          die("organize_taxf() abort!: taxid %d has different taxnames in %dth and %dth lines", taxid, t->gids[0], i);
        t->gids = realloc(t->gids, sizeof(int) * (size_t)(t->ng + 1));
        t->gids[t->ng++] = i;
        break;
      }
    }
  }
  taxon_t *tax = malloc(sizeof *tax * (size_t)(ntax + 1));
  int k = 0;
  for (int i = 0; i < tsz; i++)
    if (slots[i].taxid != -1) tax[k++] = slots[i];
  free(slots);

  char path[PATHLEN * 2 + 32];
  costat s;
  if (costat_load(in, &s) == COSTAT_ABSENT) die("cannot find cofiles.stat under %s ", in);
  const int32_t comp_num = s.comp_num, infile_num = s.infile_num;
  if (infile_num != nlines)
    die("grouping_genomes():%s's genome number %d not matches %s's genome number %d", s.path, infile_num, taxfile, nlines);
  mkdir(outdir, 0777);
  mk_setop *so;
  if (mk_setop_create(device, &so) != MK_OK) die("mk_setop_create failed: %s", mk_setop_last_error(NULL));
  uint32_t *ctx_ct = calloc((size_t)ntax + 1, 4);
  uint64_t *outidx = malloc(8 * ((size_t)ntax + 1));
  uint64_t all_ctx_ct = 0;
  int outfn = 0;
  for (int c = 0; c < comp_num; c++) {
    size_t cb = 0, ib = 0;
    uint8_t *co = need_part("grouping_genomes():", in, "combco", c, 0, &cb);
    uint8_t *idx = need_part("grouping_genomes():", in, "combco.index", c, 8 * ((size_t)infile_num + 1), &ib);
    const uint32_t *ids = (const uint32_t *)co;
    const uint64_t *pos = (const uint64_t *)idx;
    snprintf(path, sizeof path, "%s/combco.%d", outdir, c);
    FILE *f = fopen(path, "wb");
    if (!f) die("grouping_genomes():%s", path);
    uint32_t *cat = NULL;
    uint64_t cat_cap = 0, offset = 0;
    outfn = 0;
    outidx[0] = 0;
    for (int t = 0; t < ntax; t++) {
      if (tax[t].taxid == 0) continue; /* taxid 0 = leave these sketches out (:866) */
      uint64_t total = 0;
      for (int g = 0; g < tax[t].ng; g++) total += pos[tax[t].gids[g] + 1] - pos[tax[t].gids[g]];
      /* a taxon without a k-mer in this component: the reference evaluates LOG2(0 * 1.5) there (command_set.c:878: __builtin_clzll(0),
       * undefined; every build seen so far ends up with primer[0] slots and nothing in them) and writes an EMPTY block: so do we */
      if (total == 0) { outidx[++outfn] = offset; continue; }
      if (total > cat_cap) {
        if (cat) mk_host_free(cat);
        cat_cap = total + total / 4 + 1024;
        if (mk_host_alloc((void **)&cat, cat_cap * 4) != MK_OK) die("out of memory");
      }
      uint64_t w = 0;
      for (int g = 0; g < tax[t].ng; g++) {
        const uint64_t a = pos[tax[t].gids[g]], b = pos[tax[t].gids[g] + 1];
        memcpy(cat + w, ids + a, (b - a) * 4);
        w += b - a;
      }
      const uint32_t *out = NULL;
      uint64_t m = 0;
      if (mk_setop_group(so, cat, total, mk_setop_group_table_size(total), &out, &m) != MK_OK)
        die("grouping_genomes(): %s", mk_setop_last_error(so));
      if (fwrite(out, 4, m, f) != m) die("grouping_genomes():%s", path);
      offset += m; all_ctx_ct += m; ctx_ct[outfn] += (uint32_t)m;
      outidx[++outfn] = offset;
      printf("%d/%d species pangenome grouped\r", t, ntax);
    }
    printf("\n");
    fclose(f);
    if (cat) mk_host_free(cat);
    snprintf(path, sizeof path, "%s/combco.index.%d", outdir, c);
    if (!(f = fopen(path, "wb")) || fwrite(outidx, 8, (size_t)outfn + 1, f) != (size_t)outfn + 1) die("grouping_genomes():%s", path);
    fclose(f);
    free(co); free(idx);
  }
  mk_setop_destroy(so);
  /* cofiles.stat: the input's header with the new sketch count, koc = 0 and the new total (:929-966) */
  costat_set_totals(&s, outfn, 0, all_ctx_ct);
  snprintf(path, sizeof path, "%s/cofiles.stat", outdir);
  FILE *f = fopen(path, "wb");
  if (!f) die("grouping_genomes():%s", path);
  fwrite(s.raw, 1, s.hdr, f);
  fwrite(ctx_ct, 4, (size_t)outfn, f);
  for (int t = 0; t < ntax; t++) {
    if (tax[t].taxid == 0) continue;
    char name[PATHLEN];
    memset(name, 0, sizeof name);
    if (tax[t].name) snprintf(name, sizeof name, "%d_%s", tax[t].taxid, tax[t].name);
    else snprintf(name, sizeof name, "%d", tax[t].taxid);
    fwrite(name, 1, PATHLEN, f);
  }
  fclose(f);
  for (int t = 0; t < ntax; t++) { free(tax[t].name); free(tax[t].gids); }
  free(tax); free(s.raw); free(ctx_ct); free(outidx); free(txt);
  return 0;
}
/* `set -c <pan dir>...`: combin_pans(), command_set.c:515-608 -- the pan.N (or uniq_pan.N) files of several pan directories
 * become the blocks of one combined sketch directory.  File shuffling only, no device work.  The reference writes 256 bytes
 * starting at each argument string as the name record (whatever follows the NUL in argv); here the rest is zero. */
static int set_combine(int ndirs, char **dirs, const char *outdir) {
  char path[PATHLEN * 2 + 32];
  costat s0;
  if (costat_load(dirs[0], &s0) == COSTAT_ABSENT) die("combin_pans():%s", s0.path);
  const uint32_t id0 = s0.shuf_id;
  const int32_t comp_num = s0.comp_num;
  mkdir(outdir, 0777);
  uint32_t *ctx_ct = calloc((size_t)ndirs, 4);
  uint64_t all_ctx_ct = 0;
  FILE **co = malloc(sizeof(FILE *) * (size_t)comp_num), **ix = malloc(sizeof(FILE *) * (size_t)comp_num);
  uint64_t *off = calloc((size_t)comp_num, 8);
  for (int c = 0; c < comp_num; c++) {
    snprintf(path, sizeof path, "%s/combco.%d", outdir, c);
    if (!(co[c] = fopen(path, "wb"))) die("%s", path);
    snprintf(path, sizeof path, "%s/combco.index.%d", outdir, c);
    if (!(ix[c] = fopen(path, "wb"))) die("%s", path);
    fwrite(&off[c], 8, 1, ix[c]);
  }
  for (int i = 0; i < ndirs; i++) {
    costat si;
    if (costat_load(dirs[i], &si) == COSTAT_ABSENT) die("combin_pans():%s", si.path);
    free(si.raw);
    if (si.shuf_id != id0) die("combin_pans(): %dth shuf_id: %u not match 0th shuf_id: %u", i, si.shuf_id, id0);
    if (si.comp_num != comp_num) die("combin_pans(): %dth comp_num: %u not match 0th comp_num: %u", i, (unsigned)si.comp_num, (unsigned)comp_num);
    for (int c = 0; c < comp_num; c++) {
      size_t nb = 0;
      uint8_t *ids = read_part(path, sizeof path, dirs[i], "pan", c, 0, &nb);
      if (!ids) ids = read_part(path, sizeof path, dirs[i], "uniq_pan", c, 0, &nb);
      if (!ids) die("%s", path);
      fwrite(ids, 1, nb, co[c]);
      off[c] += nb / 4;
      fwrite(&off[c], 8, 1, ix[c]);
      ctx_ct[i] += (uint32_t)(nb / 4);
      free(ids);
    }
    all_ctx_ct += ctx_ct[i];
  }
  for (int c = 0; c < comp_num; c++) { fclose(co[c]); fclose(ix[c]); }
  costat_set_totals(&s0, ndirs, s0.koc, all_ctx_ct);
  snprintf(path, sizeof path, "%s/cofiles.stat", outdir);
  FILE *f = fopen(path, "wb");
  if (!f) die("%s", path);
  fwrite(s0.raw, 1, s0.hdr, f);
  fwrite(ctx_ct, 4, (size_t)ndirs, f);
  for (int i = 0; i < ndirs; i++) {
    char name[PATHLEN];
    memset(name, 0, sizeof name);
    snprintf(name, sizeof name, "%s", dirs[i]);
    fwrite(name, 1, PATHLEN, f);
  }
  fclose(f);
  free(s0.raw); free(ctx_ct); free(co); free(ix); free(off);
  return 0;
}
/* ---- `metakssd set`: -u / -q (sketch_union / uniq_sketch_union, command_set.c:241-319,427-512), -i / -s <pan>
 * (sketch_operate, :321-425), -P (print_gnames, :610-631) ----
 * The dictionary work runs on the device (mk_setop_*); the directory handling follows the reference: the 32-byte
 * cofiles.stat header is copied as it is, one pan.N / uniq_pan.N per component, and a sketch directory holding a
 * single sketch is offered for renaming in place (:254-267). */
int cmd_set(int argc, char **argv) {
  int op = -1, device = 0, print = 0; /* 0 subtract, 1 intersect, 2 union, 3 uniq_union (command_set.c:55) */
  const char *outdir = "./", *in = NULL, *panpath = NULL, *taxfile = NULL;
  for (int i = 0; i < argc; i++) {
    if (!strcmp(argv[i], "-u")) { if (op != -1) printf("set operation is already set, -u is ignored.\n"); else op = 2; }
    else if (!strcmp(argv[i], "-q")) { if (op != -1) printf("set operation is already set, -q is ignored.\n"); else op = 3; }
    else if (!strcmp(argv[i], "-s") && i + 1 < argc) { if (op != -1) printf("set operation is already set, -s is ignored.\n"); else { op = 0; panpath = argv[i + 1]; } i++; }
    else if (!strcmp(argv[i], "-i") && i + 1 < argc) { if (op != -1) printf("set operation is already set, -i is ignored.\n"); else { op = 1; panpath = argv[i + 1]; } i++; }
    else if (!strcmp(argv[i], "-c")) { if (op != -1) printf("set operation is already set, -c is ignored.\n"); else op = 4; }
    else if (!strcmp(argv[i], "-P")) print = 1;
    else if (!strcmp(argv[i], "-g") && i + 1 < argc) taxfile = argv[++i];
    else if (!strcmp(argv[i], "-o") && i + 1 < argc) outdir = argv[++i];
    else if (!strcmp(argv[i], "-p") && i + 1 < argc) ++i; /* threads: no meaning here */
    else if (!strcmp(argv[i], "--device") && i + 1 < argc) device = atoi(argv[++i]);
    else if (argv[i][0] == '-' && argv[i][1]) die("set option %s is not part of this build (-u -q -i -s -g -c -P are)", argv[i]);
    else if (!in) in = argv[i];
  }
  if (!in) usage();
  if (op == 4) { /* every non-option argument is a pan directory */
    char *dirs[4096];
    int nd = 0;
    for (int i = 0; i < argc && nd < 4096; i++) {
      if (!strcmp(argv[i], "-o") || !strcmp(argv[i], "-p") || !strcmp(argv[i], "--device")) { i++; continue; }
      if (argv[i][0] != '-') dirs[nd++] = argv[i];
    }
    return set_combine(nd, dirs, outdir);
  }
  if (op == 0 || op == 1) return set_operate(in, panpath, outdir, op == 1, device);
  if (op == -1) {
    if (print) return set_print_names(in);
    if (taxfile) return set_group(in, taxfile, outdir, device); /* looked at only without -u/-q/-i/-s (command_set.c:227-231) */
    printf("set operation use : -u, -q, -i or -s\n");
    return 255;
  }
  const char *prefix = op == 2 ? "pan" : "uniq_pan";
  const char *fn = op == 2 ? "sketch_union()" : "uniq_sketch_union()";
  char path[PATHLEN * 2 + 32];
  costat s; /* only the header is needed, and copied as it is */
  if (costat_load(in, &s) == COSTAT_ABSENT) {
    if (!s.raw) die("cannot find cofiles.stat under %s ", in);
    die("%s:%s", fn, s.path);
  }
  FILE *f;
  const int32_t comp_num = s.comp_num;
  if (s.infile_num == 1) {
    char reply = 0;
    printf("only 1 sketch, use %s as pan-sketch?(Y/N)\n", in);
    if (scanf(" %c", &reply) == 1 && (reply == 'Y' || reply == 'y')) {
      for (int c = 0; c < comp_num; c++) {
        char a[PATHLEN * 2 + 32], b[PATHLEN * 2 + 32];
        snprintf(a, sizeof a, "%s/combco.%d", in, c);
        snprintf(b, sizeof b, "%s/%s.%d", in, prefix, c);
        if (rename(a, b) != 0) die("%s: %s", fn, strerror(errno));
      }
      printf("the union directory: %s created successfully\n", in);
      return 0;
    }
  }
  mkdir(outdir, 0777);
  snprintf(path, sizeof path, "%s/cofiles.stat", outdir);
  if (!(f = fopen(path, "wb"))) die("%s:%s", fn, path);
  fwrite(s.raw, 1, s.hdr, f);
  fclose(f);
  mk_setop *so;
  if (mk_setop_create(device, &so) != MK_OK) die("mk_setop_create failed: %s", mk_setop_last_error(NULL));
  for (int c = 0; c < comp_num; c++) {
    snprintf(path, sizeof path, "%s/combco.%d", in, c);
    struct stat st;
    if (stat(path, &st) != 0) die("%s:%s", fn, path);
    const uint64_t n = (uint64_t)st.st_size / 4;
    uint32_t *ids = NULL;
    if (mk_host_alloc((void **)&ids, n ? n * 4 : 4) != MK_OK) die("out of memory");
    if (!(f = fopen(path, "rb")) || fread(ids, 4, n, f) != n) die("%s:%s", fn, path);
    fclose(f);
    const uint32_t *out = NULL;
    uint64_t m = 0;
    if (mk_setop_begin(so, op == 2 ? MK_SET_UNION : MK_SET_UNIQ_UNION) != MK_OK || mk_setop_add(so, ids, n) != MK_OK ||
        mk_setop_finish(so, &out, &m) != MK_OK)
      die("%s: %s", fn, mk_setop_last_error(so));
    mk_host_free(ids);
    snprintf(path, sizeof path, "%s/%s.%d", outdir, prefix, c);
    if (!(f = fopen(path, "wb")) || fwrite(out, 4, m, f) != m) die("%s:%s", fn, path);
    fclose(f);
  }
  mk_setop_destroy(so);
  return 0;
}
