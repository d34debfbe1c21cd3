/* cli.h -- what the files of the `metakssd` command line (metakssd_main.c, cli_*.c) share */
#ifndef MK_CLI_H
#define MK_CLI_H
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include "metakssd_hip.h"
#include "metakssd_multi.h"
#include "mk_host_internal.h" /* mk_poison_byte(): the MK_POISON test hook */

#include <dirent.h>
#include <dlfcn.h>
#include <errno.h>
#include <math.h>
#include <pthread.h>
#include <signal.h>
#include <spawn.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>

#define PATHLEN 256 /* global_basic.h:32 */
typedef struct { char **v; int n, cap; } strlist;
#define CHECK(e, call)                                                  \
  do {                                                                  \
    int _rc = (call);                                                   \
    if (_rc != MK_OK) die("%s failed (%d): %s", #call, _rc, mk_last_error(e)); \
  } while (0)

/* ---- cli_common.c ---- */
void die(const char *fmt, ...) __attribute__((noreturn));
int has_suffix(const char *s, const char *suf);
int is_fastq(const char *n);
int is_fasta(const char *n);
int is_compressed(const char *n);
void sl_push(strlist *l, const char *s);
void discover(strlist *out, int argc, char **argv);
double now_s(void);
uint8_t *read_whole(const char *path, size_t *n_out);
void *map_whole(const char *path, size_t *n);
int dir_has(const char *dir, const char *name);

/* A loaded cofiles.stat or mcofiles.stat, read-only view (the counts may be rewritten through ctx_ct / raw by who writes the file
 * back).  The loaders say how much of the file is there and never die(): every caller has its own text for each case.
 * ABSENT: not there (raw == NULL) or shorter than the header; HEADER: the counts are cut short; COUNTS: the names are cut short */
enum { COSTAT_ABSENT = 0, COSTAT_HEADER, COSTAT_COUNTS, COSTAT_FULL };
typedef struct {
  uint8_t *raw; size_t n, hdr; /* hdr: 32 (cofiles.stat) or 20 (mcofiles.stat), raw + hdr is where the counts begin */
  uint32_t shuf_id; int koc;   /* (mcofiles.stat has no koc and no all_ctx_ct) */
  int32_t kmerlen, dim_rd_len, comp_num, infile_num;
  uint64_t all_ctx_ct;
  uint32_t *ctx_ct;            /* infile_num counts */
  const char *names;           /* infile_num records of PATHLEN bytes, not always NUL-terminated */
  char path[PATHLEN * 4 + 64]; /* <dir>/cofiles.stat, for the caller's message */
} costat;
int costat_load(const char *dir, costat *s);
int mcostat_load(const char *dir, costat *s);
void costat_set_totals(costat *s, int32_t infile_num, int koc, uint64_t all_ctx_ct);
/* <dir>/<stem>.<c> whole, NULL when it is not there or shorter than `need` bytes; `path` names it either way */
uint8_t *read_part(char *path, size_t cap, const char *dir, const char *stem, int c, size_t need, size_t *n_out);
/* the same, never NULL: die("<who><path>") */
uint8_t *need_part(const char *who, const char *dir, const char *stem, int c, size_t need, size_t *n_out);

/* ---- the options of `dist` (some of them read by reverse and stage II too): filled by parse_dist_options(), metakssd_main.c ---- */
#ifndef MK_DEFAULT_AHEAD
#define MK_DEFAULT_AHEAD 0
#endif
typedef struct {
  const char *shuf_path, *outdir, *refpath, *skf; /* -L, -o, -r, -f */
  int abundance, uniq, device, quiet, timing;     /* -A, -u, --device, --quiet, --timing */
  int nthreads, threads_given, ncpu; /* -p: host threads of the front end (reference default: every processor, command_dist_wrapper.c:284-293) */
  uint64_t chunk_bytes;    /* --chunk-mib: text per framing job = about 17 MiB of rows per host-to-device copy */
  int drop_pages, inflight, slow_exit, direct_host, ascii_rows; /* --keep-pages, --inflight, --slow-exit, --direct, --ascii-rows */
  int devs[64], ndev;      /* --devices 0-7 / 0,2,5 / 0,0 (the same GPU twice: two engines, for tests) */
  int engines_per_gpu;     /* --engines 1..4: engines taking the files of a directory in turn on one GPU (default: MK_DEFAULT_ENGINES from eight files on) */
  int allow_copies;        /* --allow-device-copies: distinct GPUs whose RCCL does not come up exchange with peer copies instead of failing */
  int kmerocrs, kmerqlty;  /* -n, -Q: command_dist_wrapper.c:79-80 */
  mk_dist_opts dopt;       /* -M -O -N -D --correction: command_dist_wrapper.c:83-87 */
  int keep_shared;         /* --keepskf */
  strlist args;
  uint64_t pool_bytes;     /* --pool-mib: room for the FASTQ stream's row buffers (mk_fastq_opts::pool_bytes; 0: a few buffers, reused) */
  int mmap_input;          /* --mmap-input: the FASTQ file is mapped and the framers read the mapping (rounds 2-4) instead of pread()ing pieces */
  int early_chunks;        /* --early-chunks: chunks of a FASTQ file framed before the engine is there (mk_fastq_opts::early_chunks) */
  int frame_early;         /* --frame-early: every chunk of a FASTQ file may be framed at once, also while the runtime and the engine come up (measurement) */
  int ahead;               /* --ahead: row buffers the FASTQ stream's framers may run ahead of the pushes by */
  int no_device_inflate;   /* --no-device-inflate: BGZF inputs through `zcat -fc` like every other .gz (measurement); undoes --device-inflate */
  int gz_batches;          /* --device-inflate: single-member .gz genomes of a directory travel in gz batches and are inflated on the device.
                            * Off by default: one wavefront decodes 7 MB/s, a batch of 64 genomes of 4 MB takes 0.54 s, and sixteen zcat
                            * children are 6-14 times faster on 1 024 genomes */
  int device_inflate_q;    /* --device-inflate: a BGZF-compressed FASTQ on the -n / -Q reader (dist without -A) is inflated, framed and quality-masked on
                            * the device (mk_sketch_push_bgzf_q), 11-12 times the zcat pipe on 2 M reads.  Opt-in: without the switch this input keeps zcat */
  int device_gunzip;       /* --device-gunzip: an ordinary single-member .gz FASTQ is inflated by many wavefronts, on the -A reader (mk_sketch_push_gzip,
                            * DESIGN.md 4.14) and on the -n / -Q reader (mk_sketch_push_gzip_q).  Opt-in: without the switch such a file keeps zcat */
  int gz_gunzip;           /* --device-gunzip on a directory of genomes: the gz batches are inflated by many wavefronts per file
                            * (mk_sketch_batch_begin_gunzip); decides the genome route when --device-inflate is given too */
  int long_reads;          /* --long-reads: dist -A on FASTQ lines of any length -- the file's text goes to the device as it is and the sequence
                            * lines of complete records are scanned from the base stream (mk_sketch_push_fastq_long).  Opt-in:
                            * without the switch a line of 4 095+ characters is refused as before */
  int long_inflate;        /* --long-inflate (implies --long-reads): a .gz input of that route is inflated on the device and its text goes from HBM
                            * to the long-read framing -- a BGZF chain by mk_sketch_push_bgzf_long, another single gzip stream by
                            * mk_sketch_push_gzip_long; everything else reads as under --long-reads.  A switch of its own because
                            * --long-reads refuses --device-inflate and --device-gunzip, which name the short-read framing */
  int long_reads_q;        /* --long-reads-q: the same for the other FASTQ reader, dist without -A (-n, -Q): fastq2co's record rule and quality
                            * mask on lines of any length (mk_sketch_push_fastq_long_q).  Opt-in: without the switch a line of
                            * 19 999+ characters is refused as before */
  int long_inflate_q;      /* --long-inflate-q (implies --long-reads-q): its .gz inputs inflated on the device, by mk_sketch_push_bgzf_long_q /
                            * mk_sketch_push_gzip_long_q */
  int device_inflate_given; /* --device-inflate was on the command line (what --long-reads refuses) */
  mk_gunzip_opts gunzip_opts;   /* --gunzip-span-bytes, --gunzip-ratio, --gunzip-batch-spans (test hooks; 0 = the library's defaults) */
  uint64_t inflate_chunk_bytes; /* --inflate-chunk-kib: text bytes per chunk of the device route (test hook; 0 = the library's default) */
  int component_sz;        /* --component-sz: the reference's compile-time COMPONENT_SZ (global_basic.h:35-37) */
  int host_fasta;          /* --host-fasta: window FASTA text on the host (mk_fasta_window) instead of on the device */
  int no_batch;            /* --no-batch: genome directories file by file (the driver of round 3) */
  size_t batch_bytes;      /* --batch-mib: text per batch (0: 256 MiB where the readers pack rows, 128 MiB of text) */
  int batch_files;         /* --batch-files */
  int batch_narrow;        /* --batch-narrow: rows of 152 bases (the FASTQ rows) instead of wide rows of 240 */
  int batch_text;          /* --batch-text: the files' TEXT goes to the device (which then does the FASTA walk too) */
  const char *composite_db; /* --composite <markerdb>: dist -A hands every sample's key list to mk_composite on the device and prints the species
                            * report; no sketch directory is written */
  int abv;                 /* --abv: composite's -b (one .abv per sample instead of the report lines) */
  const char *abv_dir;     /* --abv-dir: composite's -o */
  int outdir_given, occ_given, batch_given; /* -o, -n / -Q and --batch-mib were on the command line (--composite refuses the first two) */
} cli_opts;
extern cli_opts g_opt; /* the one instance (metakssd_main.c, with the defaults) */
extern double g_t0;    /* process start (monotonic) */
void load_shuf_params(const char *shuf_path, mk_shuf *sh, mk_params *P);

/* ---- the commands ---- */
void usage(void) __attribute__((noreturn));
int cmd_set(int argc, char **argv);
int cmd_composite(int argc, char **argv);
/* cli_composite.c: one sample's rows, in print order, as the report line or (binvec) as its .abv; vec: room for ref_num + 1 entries */
typedef struct { int ref_idx; float pct; } composite_vec;
void composite_write_sample(const mk_composite_row *rows, uint64_t nrows, const char *qname, const char *refname, const char *refdir,
                            const char *outdir, int binvec, composite_vec *vec);
int cmd_shuffle(int argc, char **argv);
int cmd_reverse(int argc, char **argv);
int cmd_dist_byread(int argc, char **argv);
int run_stage2(const char *codir, const char *mcodir, int device, int quiet);
int run_combine(int ndirs, char **dirs, const char *outdir);
int run_search(const char *refdir, const char *qrydir, const char *outdir, const mk_dist_opts *o, int keep_shared, const char *skf,
               int device, int nthreads, int quiet);
int run_stage1(int stage2_after); /* cli_sketch.c: g_opt.args -> a sketch directory under g_opt.outdir, then (stage2_after) its index */
#endif
