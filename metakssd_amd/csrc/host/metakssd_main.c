/*
 * metakssd_main.c -- `metakssd` command line on top of the C ABI (host C, links libmetakssd_hip.so): usage, the command dispatch and
 * the options of `dist`.  The commands themselves: cli_sketch.c (stage I), cli_db.c, cli_set.c, cli_composite.c, cli_byread.c.
 *
 * Keeps the reference's CLI surface for the sketching path:
 *     metakssd dist -L <file.shuf> [-A] [-u] [-o outdir] [-p N] <fastq/fasta files or directories>...
 * (option table command_dist_wrapper.c:32-59, defaults :68-96, query-only branch of dist_dispatch()
 * command_dist.c:201-248, run_stageI() :341-500) and writes the same sketch directory
 * (cofiles.stat, combco.N, combco.index.N, combco.N.a).
 *
 * Also built, each on the device behind the same C ABI: FASTQ without -A (-n / -Q, fastq2co), `set`, `composite`, stage II, the
 * database search, `dist --byread` and `reverse`: see usage() and the file of each.
 *
 * Differences, all documented in DESIGN.md: inputs are processed in discovery order (the reference
 * applies a time-seeded shuffle, command_dist.c:215); --byread takes one input file; -p N sets the
 * number of host threads that read and frame/window input files ahead of the GPU (default 8); --device selects the GPU.
 */
#include "cli.h"

double g_t0;
cli_opts g_opt = {
    .outdir = ".",
    .chunk_bytes = (uint64_t)32 << 20, .drop_pages = 1, .inflight = 3,
    .kmerocrs = 1,                 /* command_dist_wrapper.c:79-80 */
    .dopt = {0, 2, 0, 0, 1.0},     /* command_dist_wrapper.c:83-87 */
    .pool_bytes = (uint64_t)6 << 30, .early_chunks = 96, .ahead = MK_DEFAULT_AHEAD,
    .component_sz = 8, .batch_files = 256,
};
/* "0-7", "0,2,5", "0,0": GPU numbers of --devices */
static int parse_devices(const char *s, int *out, int cap) {
  int n = 0;
  while (*s && n < cap) {
    char *end;
    long a = strtol(s, &end, 10);
    if (end == s || a < 0) die("--devices: cannot parse '%s'", s);
    long b = a;
    if (*end == '-') { s = end + 1; b = strtol(s, &end, 10); if (end == s || b < a) die("--devices: bad range"); }
    for (long d = a; d <= b && n < cap; d++) out[n++] = (int)d;
    s = *end == ',' ? end + 1 : end;
    if (*end && *end != ',') die("--devices: cannot parse '%s'", end);
  }
  if (n == 0) die("--devices: empty list");
  return n;
}
void usage(void) {
  fprintf(stderr,
          "usage: metakssd dist -L <file.shuf> [-A] [-u] [-n minocc] [-Q minqual] [-o outdir] [-p N] [--device D | --devices 0-7] [--engines 1..4] [--no-batch | --batch-text] <fastq|fasta|dir>...\n"
          "       metakssd dist -o <mco dir> <sketch dir>                      (stage II: inverted index)\n"
          "       metakssd dist -L <file.shuf> -r <genomes> -o <db dir>         (stage I + II)\n"
          "       metakssd dist -r <mco dir> -o <outdir> [-M 0|1] [-O 0|1|2] [-N n] [-D d] [--correction 0|1] [--keepskf] [-f skf] <sketch dir>\n"
          "       metakssd dist -L <file.shuf> --byread -o <outdir> [--device D] <one plain fasta|fastq file>   (ids per record, repeats kept)\n"
          "       metakssd reverse -L <file.shuf> [-o outdir] [-p N] [--device D] <sketch dir>   (k-mers of every sketch into <outdir>/<name>)\n"
          "       metakssd reverse -L <file.shuf> -b [--device D] <byread dir>                   (k-mers per read to stdout)\n"
          "       metakssd set -u|-q|-i <pan dir>|-s <pan dir>|-g <tax.tsv>|-c|-P [-o outdir] [--device D] <sketch dir>\n"
          "       metakssd composite -r <marker db dir> -q <-A sketch dir> [-b] [-o outdir] [--device D]\n"
          "       metakssd composite -d <x.abv>...\n"
          "       metakssd composite -r <marker db dir> -i [--device D]                 (index <dir>/abundance_Vec/*.abv)\n"
          "       metakssd composite -r <marker db dir> -s <0|1|2> [--device D] <x.abv>...  (0 cosine, 1 L1, 2 L2)\n"
          "       metakssd shuffle -k <halfK> -s <halfSubK> -l <level> [--seed N] -o <prefix>\n");
  exit(2);
}
/* the options of `dist` into g_opt; everything that is no option is an input (g_opt.args) */
static void parse_dist_options(int argc, char **argv) {
  cli_opts *o = &g_opt;
  o->nthreads = (int)sysconf(_SC_NPROCESSORS_ONLN);
  if (o->nthreads < 1) o->nthreads = 1;
  o->ncpu = o->nthreads;
  if (o->nthreads > 24) o->nthreads = 24; /* text rows: 20-24 framer threads keep PCIe busy; more only take memory bandwidth from the copies */
  for (int i = 0; i < argc; i++) {
    const int more = i + 1 < argc; /* an option's value follows */
    if (!strcmp(argv[i], "-L") && more) o->shuf_path = argv[++i];
    else if (!strcmp(argv[i], "-o") && more) { o->outdir = argv[++i]; o->outdir_given = 1; }
    else if (!strcmp(argv[i], "-p") && more) { o->nthreads = atoi(argv[++i]); o->threads_given = 1; } /* host front-end threads */
    else if (!strcmp(argv[i], "-A")) o->abundance = 1;
    else if (!strcmp(argv[i], "-u")) o->uniq = 1;
    else if (!strcmp(argv[i], "-n") && more) { /* command_dist_wrapper.c:169-180 */
      int v = atoi(argv[++i]);
      if (v > 7) { fprintf(stderr, "metakssd: -n argument is larger than Max, it has been set to 7, ignorned -n %d \n", v); v = 7; }
      else if (v < 1) { fprintf(stderr, "metakssd: -n argument is smaller than Min, it has been set to 1, ignorned -n %d \n", v); v = 1; }
      o->kmerocrs = v; o->occ_given = 1;
    }
    else if (!strcmp(argv[i], "-Q") && more) { o->kmerqlty = atoi(argv[++i]); o->occ_given = 1; } /* :182-185 */
    /* dist -L <x.shuf> -A --composite <markerdb> [--abv [--abv-dir <dir>]] [--device D] <fastq>...: the species report of
     * `composite -r <markerdb> -q <dir>` without the directory -- every sample's key list stays on the device.
     * --abv is composite's -b, --abv-dir its -o; --batch-mib is composite's (query ids per batch, 256 by default, 0: a sample a batch) */
    else if (!strcmp(argv[i], "--composite") && more) { o->composite_db = argv[++i]; o->quiet = 1; }
    else if (!strcmp(argv[i], "--abv")) o->abv = 1;
    else if (!strcmp(argv[i], "--abv-dir") && more) o->abv_dir = argv[++i];
    else if (!strcmp(argv[i], "--device") && more) o->device = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--devices") && more) o->ndev = parse_devices(argv[++i], o->devs, 64);
    else if (!strcmp(argv[i], "--engines") && more) o->engines_per_gpu = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--allow-device-copies")) o->allow_copies = 1;
    else if (!strcmp(argv[i], "--no-batch")) o->no_batch = 1;
    else if (!strcmp(argv[i], "--batch-narrow")) o->batch_narrow = 1;
    else if (!strcmp(argv[i], "--batch-text")) o->batch_text = 1;
    else if (!strcmp(argv[i], "--batch-mib") && more) { o->batch_bytes = (size_t)atoi(argv[++i]) << 20; o->batch_given = 1; }
    else if (!strcmp(argv[i], "--batch-files") && more) o->batch_files = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--host-fasta")) o->host_fasta = 1;
    else if (!strcmp(argv[i], "--quiet")) o->quiet = 1;
    else if (!strcmp(argv[i], "--component-sz") && more) o->component_sz = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--timing")) o->timing = 1;
    else if (!strcmp(argv[i], "--no-device-inflate")) { o->no_device_inflate = 1; o->gz_batches = 0; o->device_inflate_q = 0; }
    /* --device-inflate: the two opt-in device routes -- single-member .gz genomes in gz batches and a BGZF FASTQ on
     * the -n / -Q reader (4.12); the -A reader's BGZF route needs no switch.  The later of the two switches holds. */
    else if (!strcmp(argv[i], "--device-inflate")) { o->no_device_inflate = 0; o->gz_batches = 1; o->device_inflate_q = 1; o->device_inflate_given = 1; }
    else if (!strcmp(argv[i], "--long-reads")) o->long_reads = 1; /* dist -A: FASTQ lines of any length through the base stream */
    else if (!strcmp(argv[i], "--long-inflate")) o->long_reads = o->long_inflate = 1; /* ... and a .gz inflated on the device in front of it */
    else if (!strcmp(argv[i], "--long-reads-q")) o->long_reads_q = 1; /* dist -n / -Q: the same for fastq2co's reader, quality mask on the device */
    else if (!strcmp(argv[i], "--long-inflate-q")) o->long_reads_q = o->long_inflate_q = 1;
    else if (!strcmp(argv[i], "--device-gunzip")) o->device_gunzip = 1; /* dist -A and dist -n / -Q: a single-member .gz FASTQ inflated on the device */
    else if (!strcmp(argv[i], "--gunzip-members")) o->gunzip_opts.flags |= MK_GUNZIP_MEMBERS; /* ... and a concatenation of members */
    else if (!strcmp(argv[i], "--gunzip-repair")) o->gunzip_opts.flags |= MK_GUNZIP_REPAIR; /* ... with false piece starts repaired instead of a fall-back */
    else if (!strcmp(argv[i], "--gunzip-span-bytes") && more) o->gunzip_opts.span_bytes = (uint32_t)atoll(argv[++i]);
    else if (!strcmp(argv[i], "--gunzip-ratio") && more) o->gunzip_opts.ratio = (uint32_t)atoll(argv[++i]);
    else if (!strcmp(argv[i], "--gunzip-batch-spans") && more) o->gunzip_opts.batch_spans = (uint32_t)atoll(argv[++i]);
    else if (!strcmp(argv[i], "--inflate-chunk-kib") && more) o->inflate_chunk_bytes = (uint64_t)atoll(argv[++i]) << 10;
    else if (!strcmp(argv[i], "--chunk-mib") && more) o->chunk_bytes = (uint64_t)atoi(argv[++i]) << 20;
    else if (!strcmp(argv[i], "--inflight") && more) o->inflight = atoi(argv[++i]); /* row buffers queued for copying */
    else if (!strcmp(argv[i], "--frame-early")) o->frame_early = 1;
    else if (!strcmp(argv[i], "--early-chunks") && more) o->early_chunks = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--mmap-input")) o->mmap_input = 1;
    else if (!strcmp(argv[i], "--pool-mib") && more) o->pool_bytes = (uint64_t)atoll(argv[++i]) << 20;
    else if (!strcmp(argv[i], "--ahead") && more) o->ahead = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--direct")) o->direct_host = 1; /* MK_OPT_DIRECT_HOST: scan pinned row buffers in place */
    else if (!strcmp(argv[i], "--ascii-rows")) o->ascii_rows = 1; /* FASTQ rows as text (160 bytes per 150-base read) instead of packed (64) */
    else if (!strcmp(argv[i], "--slow-exit")) o->slow_exit = 1; /* destroy the engine and return from main() instead of _exit() */
    else if (!strcmp(argv[i], "--keep-pages")) o->drop_pages = 0; /* measurement: leave all unmapping to the final munmap */
    else if (!strcmp(argv[i], "-r") && more) o->refpath = argv[++i];
    else if (!strcmp(argv[i], "-M") && more) o->dopt.metric = atoi(argv[++i]);
    else if (!strcmp(argv[i], "-O") && more) o->dopt.outfields = atoi(argv[++i]);
    else if (!strcmp(argv[i], "-N") && more) o->dopt.num_neigb = atoi(argv[++i]);
    else if (!strcmp(argv[i], "-D") && more) o->dopt.dthreshold = atof(argv[++i]);
    else if (!strcmp(argv[i], "--correction") && more) o->dopt.correction = atoi(argv[++i]);
    else if (!strncmp(argv[i], "--correction=", 13)) o->dopt.correction = atoi(argv[i] + 13);
    else if (!strcmp(argv[i], "--keepskf")) o->keep_shared = 1;
    else if (!strcmp(argv[i], "-f") && more) o->skf = argv[++i];
    else if (argv[i][0] == '-' && argv[i][1]) die("option %s is not part of the sketching path built here", argv[i]);
    else sl_push(&o->args, argv[i]);
  }
}
/* dist_dispatch(), command_dist.c:49-250: what the arguments are decides the mode */
static int dist_dispatch(void) {
  cli_opts *o = &g_opt;
  strlist *args = &o->args;
  int stage2_after = 0;
  if ((o->gunzip_opts.flags & MK_GUNZIP_REPAIR) && (o->gunzip_opts.flags & MK_GUNZIP_MEMBERS))
    die("--gunzip-repair does not go with --gunzip-members: member boundaries are not repaired yet (DESIGN.md 4.22)");
  if (o->long_reads_q) { /* the long route of the -n / -Q reader: what it cannot do is said before the device is touched */
    const char *sw = o->long_inflate_q ? "--long-inflate-q" : "--long-reads-q";
    if (o->long_reads) die("%s is the route of dist without -A: not with %s", sw, o->long_inflate ? "--long-inflate" : "--long-reads");
    if (o->abundance) die("%s does not go with -A: --long-reads is the route of the counted sketch", sw);
    if (o->ndev) die("%s works on one GPU: --device D, not --devices", sw);
    if (o->composite_db) die("%s does not go with --composite: the report reads the counted sketch", sw);
    if ((o->device_inflate_given || o->device_gunzip) && o->long_inflate_q) die("--long-inflate-q chooses the device route itself: not --device-inflate or --device-gunzip");
    if (o->device_inflate_given || o->device_gunzip) die("--long-reads-q reads .gz files through zcat: not --device-inflate or --device-gunzip");
  }
  if (o->long_reads) { /* the long-read route: what it cannot do is said before the device is touched */
    const char *sw = o->long_inflate ? "--long-inflate" : "--long-reads";
    if (!o->abundance) die("%s needs -A: it is the route of the counted sketch", sw);
    if (o->occ_given) die("%s does not take -n or -Q: their reader frames lines of up to 19998 characters itself", sw);
    if (o->ndev) die("%s works on one GPU: --device D, not --devices", sw);
    if ((o->device_inflate_given || o->device_gunzip) && o->long_inflate) die("--long-inflate chooses the device route itself: not --device-inflate or --device-gunzip");
    if (o->device_inflate_given || o->device_gunzip) die("--long-reads reads .gz files through zcat: not --device-inflate or --device-gunzip");
  }
  if (o->composite_db) { /* the fused route: what it cannot do is said before the device is touched */
    if (!o->abundance) die("--composite needs -A: the report reads the k-mer counts");
    if (o->occ_given) die("--composite does not take -n or -Q: the report reads every k-mer of the reads");
    if (o->ndev) die("--composite works on one GPU: --device D, not --devices");
    if (o->engines_per_gpu > 1) die("--composite works with one engine: not --engines %d", o->engines_per_gpu);
    if (o->outdir_given) die("--composite keeps the sketch on the device; for a directory run dist -o and composite -q");
    if (!dir_has(o->composite_db, "cofiles.stat")) die("cannot find cofiles.stat under %s ", o->composite_db);
    if (!o->shuf_path) die("-L <file.shuf> is required (numeric levels generate a time-seeded table in the reference; use `metakssd shuffle`)");
    if (args->n == 0) die("please specify the input/query files");
    o->quiet = 1; o->refpath = NULL;
    return run_stage1(0);
  }
  if (o->refpath) {
    if (o->dopt.metric < 0 || o->dopt.metric > 1 || o->dopt.outfields < 0 || o->dopt.outfields > 2) die("-M takes 0/1 and -O 0/1/2");
    struct stat rst;
    if (stat(o->refpath, &rst) != 0) die("test_get_fullpath()::%s: %s", o->refpath, strerror(errno)); /* command_dist.c:321-322 */
    const int ref_co = dir_has(o->refpath, "cofiles.stat"), ref_mco = dir_has(o->refpath, "mcofiles.stat");
    if (ref_co && !ref_mco) run_stage2(o->refpath, o->refpath, o->device, o->quiet); /* :119-122: the index goes next to the sketches */
    if (ref_co || ref_mco) {
      if (args->n == 0) return 0;
      if (dir_has(args->v[0], "mcofiles.stat") && !dir_has(args->v[0], "cofiles.stat"))
        die("when -r specified, the query sould not be .mco format, the valid query format shoulde be .fas/.fq file or .co");
      if (!dir_has(args->v[0], "cofiles.stat")) die("please specify valid query genomes seq or .co file for database search");
      return run_search(o->refpath, args->v[0], o->outdir, &o->dopt, o->keep_shared, o->skf, o->device, o->nthreads, o->quiet);
    }
    /* raw sequences: stage I into outdir (no abundances, :111), then stage II in place (:112-114) */
    args->n = 0;
    sl_push(args, o->refpath);
    o->abundance = 0;
    stage2_after = 1;
  } else if (args->n >= 1 && dir_has(args->v[0], "cofiles.stat")) {
    if (args->n > 1) return run_combine(args->n, args->v, o->outdir); /* :191-194 */
    return run_stage2(args->v[0], o->outdir, o->device, o->quiet); /* :187-190 */
  }
  if (!o->shuf_path) die("-L <file.shuf> is required (numeric levels generate a time-seeded table in the reference; use `metakssd shuffle`)");
  if (args->n == 0) die("please specify the input/query files");
  return run_stage1(stage2_after);
}
int main(int argc, char **argv) {
  g_t0 = now_s();
  setvbuf(stdout, NULL, _IOLBF, 0);
  if (argc < 2) usage();
  if (!strcmp(argv[1], "shuffle")) return cmd_shuffle(argc - 2, argv + 2);
  if (!strcmp(argv[1], "set")) return cmd_set(argc - 2, argv + 2);
  if (!strcmp(argv[1], "composite")) return cmd_composite(argc - 2, argv + 2);
  if (!strcmp(argv[1], "reverse")) return cmd_reverse(argc - 2, argv + 2);
  if (strcmp(argv[1], "dist") != 0) die("only `dist`, `set`, `composite`, `reverse` and `shuffle` are part of this build (got `%s`)", argv[1]);
  for (int i = 2; i < argc; i++)
    if (!strcmp(argv[i], "--byread")) {
      for (int j = 2; j < argc; j++)
        if (!strcmp(argv[j], "--long-inflate")) die("--long-inflate does not go with --byread: per-read sketches keep the framing contract");
      for (int j = 2; j < argc; j++)
        if (!strcmp(argv[j], "--long-reads")) die("--long-reads does not go with --byread: per-read sketches keep the framing contract");
      for (int j = 2; j < argc; j++)
        if (!strcmp(argv[j], "--long-inflate-q")) die("--long-inflate-q does not go with --byread: per-read sketches keep the framing contract");
      for (int j = 2; j < argc; j++)
        if (!strcmp(argv[j], "--long-reads-q")) die("--long-reads-q does not go with --byread: per-read sketches keep the framing contract");
      return cmd_dist_byread(argc - 2, argv + 2);
    }
  parse_dist_options(argc - 2, argv + 2);
  return dist_dispatch();
}
