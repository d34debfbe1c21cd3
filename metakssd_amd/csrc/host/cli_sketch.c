/* cli_sketch.c -- stage I of `metakssd dist`: input files -> a sketch directory (run_stageI(), command_dist.c:341-500).  The whole host
 * hot path lives in this one file: the engine start-up, the FASTQ / BGZF / gunzip / FASTA routes, the pinner, the prefetch workers,
 * the batch readers, and the four file loops (batches, files sharded over GPUs, several engines on one GPU, serial). */
#include "cli.h"

#define IOBUF ((size_t)64 << 20)
#define ROWBUF ((size_t)64 << 20)

/* The engine is created on a helper thread (HIP start-up, 2 GB of tables, the .shuf upload) while the main thread maps the
 * input and starts framing; whoever needs the engine first waits for it here. */
typedef struct {
  pthread_t th;
  pthread_mutex_t mu;
  pthread_cond_t cv;
  int done, rc, device;
  int ndev, devs[64];   /* --devices: more than one GPU -> libmetakssd_multi.so */
  unsigned multi_flags; /* MK_MULTI_ALLOW_DEVICE_COPIES with --allow-device-copies */
  mk_multi *multi;
  int lazy_tables;      /* MK_ENGINE_LAZY_TABLES: the inputs look like a directory of genomes for batches (set before have_params) */
  int have_params;      /* the main thread has read the .shuf file: P may be used */
  const mk_params *P;
  mk_engine *eng;
  char err[512];
  double t_start, t_hip_ready, t_ready; /* seconds since process start */
} engine_future;
/* libmetakssd_multi.so (it links librccl.so, 570 MB) is loaded only when --devices names several GPUs */
static struct {
  int (*create)(const mk_params *, const int *, int, unsigned, mk_multi **);
  const char *(*last_error)(const mk_multi *);
  mk_engine *(*engine)(mk_multi *, int);
  const char *(*transport)(const mk_multi *);
  int (*begin)(mk_multi *, int);
  int (*begin_occ)(mk_multi *, int);
  int (*finish)(mk_multi *, mk_result *, double *, double *);
} g_multi;
static void load_multi(void) {
  void *h = dlopen("libmetakssd_multi.so", RTLD_NOW | RTLD_GLOBAL);
  if (!h) die("--devices with several GPUs needs libmetakssd_multi.so: %s", dlerror());
  *(void **)&g_multi.create = dlsym(h, "mk_multi_create_ex");
  *(void **)&g_multi.last_error = dlsym(h, "mk_multi_last_error");
  *(void **)&g_multi.engine = dlsym(h, "mk_multi_engine");
  *(void **)&g_multi.transport = dlsym(h, "mk_multi_transport");
  *(void **)&g_multi.begin = dlsym(h, "mk_multi_begin");
  *(void **)&g_multi.begin_occ = dlsym(h, "mk_multi_begin_occ");
  *(void **)&g_multi.finish = dlsym(h, "mk_multi_finish");
  if (!g_multi.create || !g_multi.last_error || !g_multi.engine || !g_multi.transport || !g_multi.begin || !g_multi.begin_occ || !g_multi.finish)
    die("libmetakssd_multi.so: missing symbols");
}
typedef struct {
  engine_future *fut;
  mk_engine *eng; /* NULL until engine_get(); with several GPUs: engine 0, where the sketch is finished */
  mk_multi *multi;
  int ndev;
  mk_engine *engs[64];
  uint64_t rr;    /* row buffers dealt so far (round-robin over the engines) */
  double gather_ms, tail_ms;
  uint8_t *io;   /* raw text */
  uint8_t *rows; /* pinned rows */
  uint64_t next_ordinal;
  uint64_t nrows_total;
  int occ;      /* FASTQ without -A: fastq2co()'s reader (quality mask, its record rule) */
  int qmin, TL; /* -Q, k-mer length */
  int nthreads; /* host threads for framing one big FASTQ (mk_fastq_frame_mt) */
  /* the sketch the current file goes into: begun lazily, by whoever pushes first */
  int begun, mode, min_occ;
  uint64_t chunk_bytes;
  mk_fastq_stats fq_stats;
  double t_first_push, t_last_push, t_unmapped, t_begin_s;
  int drop_pages, inflight, direct_host, packed;
  uint8_t *arena; /* row-buffer pool of the FASTQ stream: an anonymous mapping, pinned piece by piece behind the framers (pin_*) */
  size_t arena_bytes;
  struct pinner *pin;
  int want_keys; /* dist -A --composite: the finish ends at the engine's key list (mk_sketch_finish_keys), which keys / kcnt / nkeys then name */
  const uint64_t *keys;
  const uint32_t *kcnt;
  uint64_t nkeys;
  uint8_t *long_buf[2]; /* --long-reads: two pinned text buffers, filled in turn (sketch_fastq_long) */
  int bgzf_ok; /* one engine on one GPU: a BGZF-compressed FASTQ is inflated on the device (sketch_fastq_bgzf): on the -A reader by default,
                * on the -n / -Q reader with --device-inflate */
} ctx_t;
static void *engine_thread(void *arg) {
  engine_future *f = arg;
  int n = 0;
  f->t_start = now_s() - g_t0;
  int rc = mk_device_count(&n); /* first HIP call of the process: runtime start-up, while the main thread reads the .shuf file */
  f->t_hip_ready = now_s() - g_t0;
  pthread_mutex_lock(&f->mu);
  while (!f->have_params) pthread_cond_wait(&f->cv, &f->mu);
  pthread_mutex_unlock(&f->mu);
  if (rc == MK_OK && !f->P) rc = MK_ERR_ARG; /* the main thread gave up */
  if (rc == MK_OK && f->ndev > 1) {
    rc = g_multi.create(f->P, f->devs, f->ndev, f->multi_flags, &f->multi);
    if (rc != MK_OK) snprintf(f->err, sizeof f->err, "%s", g_multi.last_error(NULL));
    else f->eng = g_multi.engine(f->multi, 0);
  } else if (rc == MK_OK) {
    rc = mk_engine_create_ex(f->P, f->device, f->lazy_tables ? MK_ENGINE_LAZY_TABLES : 0u, &f->eng);
    if (rc != MK_OK) snprintf(f->err, sizeof f->err, "%s", mk_last_error(NULL));
  } else snprintf(f->err, sizeof f->err, "%s", mk_last_error(NULL));
  f->t_ready = now_s() - g_t0;
  pthread_mutex_lock(&f->mu);
  f->rc = rc;
  f->done = 1;
  pthread_cond_broadcast(&f->cv);
  pthread_mutex_unlock(&f->mu);
  return NULL;
}
static void engine_start(engine_future *f, int device, const int *devs, int ndev, unsigned multi_flags) {
  memset(f, 0, sizeof *f);
  f->device = device;
  f->ndev = ndev;
  f->multi_flags = multi_flags;
  for (int i = 0; i < ndev && i < 64; i++) f->devs[i] = devs[i];
  if (ndev > 1) load_multi();
  pthread_mutex_init(&f->mu, NULL);
  pthread_cond_init(&f->cv, NULL);
  if (pthread_create(&f->th, NULL, engine_thread, f) != 0) die("cannot start a thread: %s", strerror(errno));
}
static void engine_params(engine_future *f, const mk_params *P) {
  pthread_mutex_lock(&f->mu);
  f->P = P;
  f->have_params = 1;
  pthread_cond_broadcast(&f->cv);
  pthread_mutex_unlock(&f->mu);
}
/* the per-engine options of the command line, for every engine that is attached to a ctx (the start-up engine, the extra engines
 * of --engines, the drivers' engines of --devices) */
static void engine_apply_options(const ctx_t *c, mk_engine *e) {
  if (c->direct_host) mk_engine_set_option(e, MK_OPT_DIRECT_HOST, 1);
  /* test hook: MK_BATCH_TAB_BITS=<9..22> gives every file of a batch a table of that size (MK_OPT_BATCH_TAB_BITS), so that files
   * overflow it and take the sketched-alone path of mk_sketch_batch_end */
  if (getenv("MK_BATCH_TAB_BITS")) mk_engine_set_option(e, MK_OPT_BATCH_TAB_BITS, atoi(getenv("MK_BATCH_TAB_BITS")));
  /* test hook: MK_BATCH_HOME_IDS=<4..> lets at most that many ids come home with a batch (MK_OPT_BATCH_HOME_IDS), so that
   * mk_sketch_batch_end fetches the rest by its late copy */
  if (getenv("MK_BATCH_HOME_IDS")) mk_engine_set_option(e, MK_OPT_BATCH_HOME_IDS, atoi(getenv("MK_BATCH_HOME_IDS")));
}
static mk_engine *engine_get(ctx_t *c) {
  if (c->eng) return c->eng;
  engine_future *f = c->fut;
  pthread_mutex_lock(&f->mu);
  while (!f->done) pthread_cond_wait(&f->cv, &f->mu);
  pthread_mutex_unlock(&f->mu);
  if (f->rc != MK_OK) die("mk_engine_create failed (%d): %s", f->rc, f->err);
  c->eng = f->eng;
  c->multi = f->multi;
  c->ndev = f->multi ? f->ndev : 1;
  for (int i = 0; i < c->ndev; i++) c->engs[i] = f->multi ? g_multi.engine(f->multi, i) : f->eng;
  for (int i = 0; i < c->ndev; i++) engine_apply_options(c, c->engs[i]);
  return c->eng;
}
/* mk_sketch_begin for the current file, once, at the first push (or at finish for an input without rows) */
static mk_engine *sketch_engine(ctx_t *c) {
  mk_engine *e = engine_get(c);
  if (!c->begun) {
    const double tb = now_s();
    if (c->multi) {
      const int rc = c->mode == MK_MODE_OCC_SET ? g_multi.begin_occ(c->multi, c->min_occ) : g_multi.begin(c->multi, c->mode);
      if (rc != MK_OK) die("mk_multi_begin failed (%d): %s", rc, g_multi.last_error(c->multi));
    } else if (c->mode == MK_MODE_OCC_SET) CHECK(e, mk_sketch_begin_occ(e, c->min_occ)); /* command_dist.c:385-386 */
    else CHECK(e, mk_sketch_begin(e, c->mode));
    c->t_begin_s += now_s() - tb;
    c->begun = 1;
  }
  return e;
}
/* input opened like the reference does: through `zcat -fc` when compressed (iseq2comem.c:216,666-669), directly otherwise
 * (same bytes, no child process).  zcat is started with an argument vector, not through a shell: a file name is never
 * interpreted; its exit status is checked when the input is closed (a corrupt .gz must not yield a silently short sketch). */
typedef struct { FILE *f; pid_t pid; const char *path; } input_t;

static int open_input(const char *path, input_t *in) {
  in->pid = 0; in->path = path; in->f = NULL;
  if (!is_compressed(path)) { in->f = fopen(path, "rb"); return in->f != NULL; }
  int fd[2];
  if (pipe(fd) != 0) return 0;
  /* posix_spawnp, not fork: the process is heavily threaded and holds a live HIP runtime by the time genomes are read (worker
   * threads beside the engines); a spawned child takes none of that state along */
  posix_spawn_file_actions_t fa;
  if (posix_spawn_file_actions_init(&fa) != 0) { close(fd[0]); close(fd[1]); return 0; }
  posix_spawn_file_actions_adddup2(&fa, fd[1], 1);
  posix_spawn_file_actions_addclose(&fa, fd[0]);
  posix_spawn_file_actions_addclose(&fa, fd[1]);
  char *const zargv[] = {(char *)"zcat", (char *)"-fc", (char *)"--", (char *)path, NULL};
  pid_t pid = 0;
  const int src = posix_spawnp(&pid, "zcat", &fa, NULL, zargv, environ);
  posix_spawn_file_actions_destroy(&fa);
  if (src != 0) { close(fd[0]); close(fd[1]); errno = src; return 0; }
  close(fd[1]);
  in->pid = pid;
  in->f = fdopen(fd[0], "rb");
  return in->f != NULL;
}
static void close_input(input_t *in) {
  if (in->f) fclose(in->f);
  if (in->pid > 0) {
    int st = 0;
    if (waitpid(in->pid, &st, 0) < 0 || !WIFEXITED(st) || WEXITSTATUS(st) != 0)
      die("%s: `zcat -fc` failed (status %d): the input was not read completely", in->path, WIFEXITED(st) ? WEXITSTATUS(st) : -1);
  }
}
/* buffers of the windowed paths (pipes, FASTA); a mapped FASTQ file does not need them */
/* MK_POISON (mk_host_internal.h): a pool buffer taken back for another file / batch is overwritten with the pattern first */
static void repoison(void *p, size_t n) { const int pz = mk_poison_byte(); if (pz >= 0 && p && n) memset(p, pz, n); }

static void ensure_buffers(ctx_t *c) {
  if (c->io) return;
  c->io = malloc(IOBUF);
  if (!c->io || mk_host_alloc((void **)&c->rows, ROWBUF) != MK_OK) die("out of memory");
}
static void push_rows(ctx_t *c, const uint8_t *rows, uint32_t stride, uint64_t nrows) {
  mk_engine *e = sketch_engine(c);
  CHECK(e, mk_sketch_push_reads(e, rows, stride, nrows, c->next_ordinal));
  c->next_ordinal += nrows;
  c->nrows_total += nrows;
  if (rows == c->rows) repoison(c->rows, ROWBUF); /* (push returned: the rows have been copied) */
}
/* ---- the row-buffer arena is pinned PIECE BY PIECE, behind the framers and in front of the pushes -----------------------------
 * The arena has room for the whole file's rows (mk_fastq_opts::pool_bytes), so that the framers run at their own pace from the first
 * moment -- also through the 80-110 ms in which the HIP runtime and the engine come up and nothing can be pinned or pushed.  Pinning
 * all of it up front would cost more than it saves (fresh pages pin at 5 GB/s, and pinning beside the creation of the engine's queue
 * makes that three times as long); pages the framers have WRITTEN pin at over 100 GB/s.  So: a framer reports a finished buffer
 * (mk_rows_sink::ready); a pinner thread -- idle until the engine is there -- registers runs of finished buffers that lie side by
 * side (up to 256 MiB a call); a push waits until its buffer is pinned.  The pinner is twice as fast as the link, so after its first
 * call it stays in front of the pushes.  A registration always ends at a buffer's end: a copy whose source lies across two
 * registrations is refused by the runtime (invalid argument), so the unit is the buffer, and a new file -- whose buffers may have
 * another size -- starts from nothing pinned (pin_reset). */
#define PIN_RUN_BYTES ((size_t)256 << 20)
typedef struct pinner {
  uint8_t *base;
  size_t bytes, buf_bytes, nbuf;  /* buf_bytes: learnt from the first report after a reset (all buffers of a stream have one size) */
  size_t kept_buf_bytes;          /* the size the standing registrations and states were made for */
  uint8_t *state;                 /* per buffer: 0 fresh, 1 written (may be pinned), 2 pinned */
  size_t state_cap;
  void **regs; int nregs, regs_cap; /* bases of the registrations made (to undo them) */
  int device, go, stop, started, busy;
  pthread_t th;
  pthread_mutex_t mu;
  pthread_cond_t cv_work, cv_pinned;
  double t_pin_s; int calls; size_t pinned_bytes;
} pinner;
static void *pinner_run(void *arg) {
  pinner *p = arg;
  pthread_mutex_lock(&p->mu);
  for (;;) {
    size_t b0 = p->nbuf;
    if (p->go) for (size_t b = 0; b < p->nbuf; b++) if (p->state[b] == 1) { b0 = b; break; }
    if (p->stop) break;
    if (b0 == p->nbuf) { pthread_cond_wait(&p->cv_work, &p->mu); continue; }
    size_t b1 = b0;
    while (b1 < p->nbuf && (b1 - b0 + 1) * p->buf_bytes <= PIN_RUN_BYTES + p->buf_bytes && p->state[b1] == 1) b1++;
    uint8_t *at = p->base + b0 * p->buf_bytes;
    const size_t len = (b1 - b0) * p->buf_bytes;
    p->busy = 1;
    pthread_mutex_unlock(&p->mu);
    const double t0 = now_s();
    if (mk_host_register_on(p->device, at, len) != MK_OK) die("pinning the row buffers failed: %s", mk_last_error(NULL));
    const double dt = now_s() - t0;
    pthread_mutex_lock(&p->mu);
    p->busy = 0;
    for (size_t b = b0; b < b1; b++) p->state[b] = 2;
    if (p->nregs == p->regs_cap) {
      p->regs_cap = p->regs_cap ? 2 * p->regs_cap : 64;
      p->regs = realloc(p->regs, sizeof(void *) * (size_t)p->regs_cap);
      if (!p->regs) die("out of memory");
    }
    p->regs[p->nregs++] = at;
    p->t_pin_s += dt; p->calls++; p->pinned_bytes += len;
    pthread_cond_broadcast(&p->cv_pinned);
  }
  pthread_mutex_unlock(&p->mu);
  return NULL;
}
/* the buffer at `at` (room `bytes`): its index; the first report after a reset fixes the buffers' size.  Called with the lock held. */
static size_t pin_index(pinner *p, const uint8_t *at, size_t bytes) {
  if (!p->buf_bytes && bytes == p->kept_buf_bytes && p->nbuf) { /* the same layout as the last stream's: its pins stand */
    p->buf_bytes = bytes;
    for (size_t b = 0; b < p->nbuf; b++) if (p->state[b] == 1) p->state[b] = 0; /* (written by the last stream, never pushed: to be written again) */
  }
  if (!p->buf_bytes) {
    /* another layout: a registration must not lie across a buffer's end, so the old ones go (the pinner is idle: go == 0) */
    for (int i = 0; i < p->nregs; i++) mk_host_unregister(p->regs[i]);
    p->nregs = 0;
    p->kept_buf_bytes = bytes;
    p->buf_bytes = bytes;
    p->nbuf = p->bytes / bytes;
    if (p->nbuf > p->state_cap) {
      free(p->state);
      p->state = calloc(p->nbuf, 1);
      if (!p->state) die("out of memory");
      p->state_cap = p->nbuf;
    } else memset(p->state, 0, p->nbuf);
  }
  if (bytes != p->buf_bytes || (size_t)(at - p->base) % p->buf_bytes) die("internal: row buffers of two sizes in one stream");
  return (size_t)(at - p->base) / p->buf_bytes;
}
static void pin_mark(pinner *p, const uint8_t *at, size_t bytes) { /* the buffer at `at` has been written: it may be pinned */
  if (!p || at < p->base || bytes == 0) return;
  pthread_mutex_lock(&p->mu);
  const size_t b = pin_index(p, at, bytes);
  if (b < p->nbuf && p->state[b] == 0) { p->state[b] = 1; if (p->go) pthread_cond_signal(&p->cv_work); }
  pthread_mutex_unlock(&p->mu);
}
static void pin_wait(pinner *p, const uint8_t *at) { /* returns when the buffer at `at` is pinned; lets the pinner loose */
  if (!p || at < p->base) return;
  pthread_mutex_lock(&p->mu);
  if (!p->buf_bytes) die("internal: a push before any row buffer was reported");
  const size_t b = (size_t)(at - p->base) / p->buf_bytes;
  if (b < p->nbuf) {
    if (p->state[b] == 0) p->state[b] = 1;
    p->go = 1;
    pthread_cond_signal(&p->cv_work);
    while (p->state[b] != 2) pthread_cond_wait(&p->cv_pinned, &p->mu);
  }
  pthread_mutex_unlock(&p->mu);
}
static void pin_reset(pinner *p) { /* a new stream into the same arena: its buffers may have another size (pin_index decides) */
  if (!p) return;
  pthread_mutex_lock(&p->mu);
  p->go = 0;
  while (p->busy) pthread_cond_wait(&p->cv_pinned, &p->mu);
  p->buf_bytes = 0;
  pthread_mutex_unlock(&p->mu);
}
static void pin_destroy(pinner *p) { /* registrations undone, thread gone (the mapping is the caller's) */
  if (!p) return;
  pthread_mutex_lock(&p->mu);
  p->stop = 1;
  pthread_cond_broadcast(&p->cv_work);
  pthread_mutex_unlock(&p->mu);
  if (p->started) pthread_join(p->th, NULL);
  for (int i = 0; i < p->nregs; i++) mk_host_unregister(p->regs[i]);
  free(p->regs); free(p->state);
  pthread_mutex_destroy(&p->mu); pthread_cond_destroy(&p->cv_work); pthread_cond_destroy(&p->cv_pinned);
  free(p);
}
static pinner *pin_create(uint8_t *base, size_t bytes, int device) {
  pinner *p = calloc(1, sizeof *p);
  if (!p) return NULL;
  p->base = base; p->bytes = bytes; p->device = device;
  pthread_mutex_init(&p->mu, NULL); pthread_cond_init(&p->cv_work, NULL); pthread_cond_init(&p->cv_pinned, NULL);
  if (pthread_create(&p->th, NULL, pinner_run, p) != 0) { free(p); return NULL; }
  p->started = 1;
  return p;
}
/* ---- sink of the whole-file FASTQ stream: pinned buffers, asynchronous pushes, the engine awaited at the first push ---- */
static void cli_sink_ready(void *ctx, const uint8_t *rows, size_t bytes) { pin_mark(((ctx_t *)ctx)->pin, rows, bytes); }
static int cli_sink_push(void *ctx, const uint8_t *rows, uint32_t stride, uint64_t nrows, uint64_t ord, uint64_t *token) {
  ctx_t *c = ctx;
  (void)sketch_engine(c);
  /* the engine is there, i.e. the runtime is up: the pinner may work; this buffer's pages before anything else */
  pin_wait(c->pin, rows);
  if (c->t_first_push == 0) c->t_first_push = now_s() - g_t0;
  /* several GPUs: the row buffers are dealt round-robin, so that every GPU's PCIe link carries a share at any time;
   * ordinals are global, so it does not matter which engine sees which rows */
  const int k = (int)(c->rr++ % (uint64_t)c->ndev);
  uint64_t t = 0;
  const int rc = mk_sketch_push_reads_async(c->engs[k], rows, stride, nrows, ord, &t);
  if (rc != MK_OK && c->ndev > 1) fprintf(stderr, "metakssd: GPU %d: %s\n", k, mk_last_error(c->engs[k]));
  *token = t * 64u + (uint64_t)k;
  return rc;
}
static int cli_sink_wait(void *ctx, uint64_t token) { return mk_sketch_push_wait(((ctx_t *)ctx)->engs[token % 64u], token / 64u); }
/* the row-buffer pool while the HIP runtime is still coming up: the same mapping mk_host_arena_alloc makes (2 MiB granules,
 * huge pages asked for, touched by eight threads), not pinned yet -- the framers fill it while the runtime and the engine start,
 * and the first push pins it (cli_sink_push) */
typedef struct { uint8_t *p; size_t n; } touch_job;
static void *touch_run(void *arg) {
  touch_job *j = arg;
  for (size_t off = 0; off < j->n; off += 4096) j->p[off] = 0;
  return NULL;
}
static uint8_t *arena_map_untouched(size_t bytes, size_t *len_out) {
  const size_t huge = (size_t)2 << 20;
  const size_t len = (bytes + huge - 1) & ~(huge - 1);
  uint8_t *m = mmap(NULL, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (m == MAP_FAILED) return NULL;
#ifdef MADV_HUGEPAGE
  (void)madvise(m, len, MADV_HUGEPAGE);
#endif
  *len_out = len;
  return m;
}
static uint8_t *arena_map_unpinned(size_t bytes, size_t *len_out) {
  size_t len = 0;
  uint8_t *m = arena_map_untouched(bytes, &len);
  if (!m) return NULL;
  enum { T = 8 };
  touch_job job[T];
  pthread_t th[T];
  int started = 0;
  for (int t = 0; t < T; t++) {
    const size_t lo = len / T * (size_t)t, hi = t + 1 == T ? len : len / T * (size_t)(t + 1);
    job[t].p = m + lo; job[t].n = hi - lo;
    if (t + 1 < T && pthread_create(&th[t], NULL, touch_run, &job[t]) == 0) started |= 1 << t;
    else touch_run(&job[t]);
  }
  for (int t = 0; t < T; t++) if (started & (1 << t)) pthread_join(th[t], NULL);
  *len_out = len;
  return m;
}
static uint8_t *cli_sink_alloc(void *ctx, size_t bytes) { /* the arena (and what is pinned of it) is kept for the next file and goes with the process */
  ctx_t *c = ctx;
  if (c->arena && c->arena_bytes >= bytes) { pin_reset(c->pin); return c->arena; } /* (MK_POISON: the stream fills every buffer it takes) */
  if (c->pin) { pin_destroy(c->pin); c->pin = NULL; }
  if (c->arena) munmap(c->arena, c->arena_bytes);
  c->arena = NULL; c->arena_bytes = 0;
  /* an untouched anonymous mapping (2 MiB granules, huge pages asked for): the framers' stores bring the pages in, the pinner
   * registers them once they are written -- nothing here waits for the engine or costs anything for room that is never used */
  size_t len = 0;
  uint8_t *m = arena_map_untouched(bytes, &len);
  if (!m) return NULL;
  c->pin = pin_create(m, len, c->fut ? (c->fut->ndev > 1 ? c->fut->devs[0] : c->fut->device) : 0);
  if (!c->pin) { munmap(m, len); return NULL; }
  c->arena = m; c->arena_bytes = len;
  return m;
}
static void cli_sink_release(void *ctx, uint8_t *p, size_t bytes) { (void)ctx; (void)p; (void)bytes; }

/* an uncompressed regular file is framed straight out of its page-cache mapping by the whole-file stream
 * (mk_fastq_stream.c): no copy into an I/O buffer, `-p` threads fault the pages in and frame concurrently, the buffers
 * go to the engine in file order while later chunks are still being framed */
static int sketch_fastq_mapped(ctx_t *c, const char *path) {
  if (is_compressed(path)) return 0;
  int fd = open(path, O_RDONLY);
  if (fd < 0) return 0;
  struct stat st;
  if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size == 0) { close(fd); return 0; }
  const size_t size = (size_t)st.st_size;
  /* the framers pread the file piece by piece (mk_fastq_opts::fd): nothing of it is mapped into this process, so thirty-two threads
   * at memory speed cause no page-table work and no TLB shoot-downs beside the HIP runtime's start-up.  --mmap-input: the mapping of
   * rounds 2-4 (populated and dropped chunk by chunk by the framers), for comparison */
  const uint8_t *map = NULL;
  if (g_opt.mmap_input) {
    map = mmap(NULL, size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    fd = -1;
    if (map == MAP_FAILED) return 0;
  }
  mk_fastq_opts o;
  memset(&o, 0, sizeof o);
  o.occ = c->occ; o.qmin = c->qmin; o.TL = c->TL;
  o.nthreads = c->nthreads; o.inflight = c->inflight; o.chunk_bytes = c->chunk_bytes; o.ahead = g_opt.ahead;
  o.packed = c->packed; /* reads of up to 152 bases cross PCIe as 64-byte packed rows (geometries with a tuned scan kernel) */
  o.drop_pages = c->drop_pages; /* a private read-only file mapping that is unmapped below */
  o.pool_bytes = g_opt.pool_bytes;
  o.fd = map ? 0 : fd;
  /* while the HIP runtime and the engine come up only a handful of chunks are framed (thirty-two framers at memory speed make that
   * start-up two to eight times as long, profiles/r05_e2e_front_end.txt); the rest from the moment the first buffer has been pushed */
  o.early_chunks = g_opt.frame_early ? 0 : g_opt.early_chunks;
  mk_rows_sink sink = {c, cli_sink_push, cli_sink_wait, cli_sink_alloc, cli_sink_release, cli_sink_ready};
  mk_fastq_stats fs;
  /* the framers start at once, into a pool that is pinned when the engine is there (cli_sink_alloc / cli_sink_push): the
   * engine's queue creation takes three times as long (45 ms instead of 14) when it runs into the driver together with the
   * pinning, so the pinning waits for it -- the framing does not */
  const int rc = mk_fastq_stream(map, size, &o, &sink, c->next_ordinal, &fs);
  if (rc == MK_ERR_ARG || rc == MK_ERR_FORMAT)
    die("%s: FASTQ line longer than the reference's fgets() width (%s): outside the framing contract", path,
        c->occ ? "19998 characters, iseq2comem.c:319,343" : "4094 characters, iseq2comem.c:656,673");
  if (rc != MK_OK) {
    engine_get(c); /* no usable device: say that (pinned buffers cannot be had either), not "out of memory" */
    die("mk_fastq_stream failed (%d): %s", rc, mk_last_error(c->eng));
  }
  c->next_ordinal += fs.rows;
  c->nrows_total += fs.rows;
  c->fq_stats = fs;
  c->t_last_push = now_s() - g_t0;
  if (map) munmap((void *)map, size);
  else close(fd);
  c->t_unmapped = now_s() - g_t0;
  return 1;
}
/* --timing: which way a compressed input went, one JSON line per input.  g_gz_fallback: the device route was tried first and gave
 * this inflate status (a gzip genome that came back from its batch, see the batch driver) */
static const char *g_gz_fallback = NULL;
static void report_route(const char *path, const char *route, const mk_bgzf_stats *bs) {
  if (!g_opt.timing) return;
  char fb[160] = "";
  if (g_gz_fallback) snprintf(fb, sizeof fb, ", \"fallback\": \"%s\"", g_gz_fallback);
  printf("{\"input\": \"%s\", \"route\": \"%s\", \"blocks\": %llu, \"chunks\": %llu, \"comp_bytes\": %llu, \"text_bytes\": %llu, \"rows\": %llu, "
         "\"inflate_ms\": %.3f, \"frame_ms\": %.3f, \"bgzf_scan_s\": %.4f, \"read_s\": %.4f, \"route_total_s\": %.4f%s}\n",
         path, route, bs ? (unsigned long long)bs->blocks : 0ull, bs ? (unsigned long long)bs->chunks : 0ull, bs ? (unsigned long long)bs->comp_bytes : 0ull,
         bs ? (unsigned long long)bs->text_bytes : 0ull, bs ? (unsigned long long)bs->rows : 0ull, bs ? bs->inflate_ms : 0.0, bs ? bs->frame_ms : 0.0,
         bs ? bs->t_scan_s : 0.0, bs ? bs->t_read_s : 0.0, bs ? bs->t_total_s : 0.0, fb);
}
/* the device route gave an input up: what it pushed is finished and dropped, the next push begins anew, --timing names the reason */
static void drop_pushed_and_fall_back(ctx_t *c, mk_engine *e, const char *why) {
  mk_result dropped;
  const int frc = mk_sketch_finish(e, &dropped);
  if (frc != MK_OK && frc != MK_ERR_CROWDED) die("mk_sketch_finish failed (%d): %s", frc, mk_last_error(e));
  if (frc == MK_OK) mk_result_release(e, &dropped);
  c->begun = 0;
  g_gz_fallback = why;
}
/* a .gz that is a BGZF chain from its first byte to its last (mk_bgzf_scan) is inflated, checked and framed on the device; 0: not
 * such a file, the caller goes on with `zcat -fc`, with today's behaviour and messages.  The -n / -Q reader (c->occ) takes this
 * route only with --device-inflate, and a file with a line of 4095+ characters -- which fastq2co() reads (iseq2comem.c:319,343) and
 * the device does not cut into windows -- comes back from it: what has been pushed is finished and dropped, the caller begins the
 * sketch anew and reads the file from its start through `zcat -fc`; --timing says so ("fallback": "long line"). */
static int sketch_fastq_bgzf(ctx_t *c, const char *path) {
  if (!c->bgzf_ok || (c->occ && !g_opt.device_inflate_q) || g_opt.no_device_inflate || !has_suffix(path, ".gz")) return 0;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return 0;
  struct stat st;
  if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size == 0) { close(fd); return 0; }
  mk_bgzf_block *tab = NULL;
  uint64_t nb = 0, total = 0;
  int is_bgzf = 0;
  if (mk_bgzf_scan(fd, NULL, (size_t)st.st_size, &tab, &nb, &total, &is_bgzf) != MK_OK || !is_bgzf) { close(fd); return 0; }
  mk_bgzf_free(tab);
  mk_engine *e = sketch_engine(c);
  if (c->t_first_push == 0) c->t_first_push = now_s() - g_t0;
  mk_bgzf_opts o;
  memset(&o, 0, sizeof o);
  o.chunk_bytes = g_opt.inflate_chunk_bytes;
  mk_bgzf_stats bs;
  const int rc = c->occ ? mk_sketch_push_bgzf_q(e, fd, (size_t)st.st_size, &o, c->qmin, c->next_ordinal, &bs)
                        : mk_sketch_push_bgzf(e, fd, (size_t)st.st_size, &o, c->next_ordinal, &bs);
  close(fd);
  if (rc == MK_ERR_FORMAT && bs.bad_block >= 0)
    die("%s: BGZF block %lld is damaged (%s): the input was not read completely", path, (long long)bs.bad_block, mk_inflate_status_text(bs.bad_status));
  if (rc == MK_ERR_FORMAT && c->occ) {
    drop_pushed_and_fall_back(c, e, "long line");
    return 0;
  }
  if (rc == MK_ERR_FORMAT)
    die("%s: FASTQ line longer than the reference's fgets() width (%s): outside the framing contract", path, "4094 characters, iseq2comem.c:656,673");
  if (rc != MK_OK) die("%s failed (%d): %s", c->occ ? "mk_sketch_push_bgzf_q" : "mk_sketch_push_bgzf", rc, mk_bgzf_last_error());
  c->next_ordinal += bs.rows;
  c->nrows_total += bs.rows;
  c->t_last_push = now_s() - g_t0;
  report_route(path, "device-inflate", &bs);
  return 1;
}
/* --device-gunzip: a .gz that is ONE gzip member (mk_gzip_scan_stream; a BGZF file has gone its own way before) is inflated, checked
 * and framed on the device, for the -A reader and for the -n / -Q reader (c->occ: mk_sketch_push_gzip_q with c->qmin).  0: not such
 * a file, or the device route gave it up with a status or a line of 4095+ characters -- then what was pushed is finished and
 * dropped, the caller begins the sketch anew and reads the file from its start through `zcat -fc`, which alone decides whether
 * the file is damaged; --timing says so ("fallback": the status, or "long line"). */
static int sketch_fastq_gunzip(ctx_t *c, const char *path) {
  if (!g_opt.device_gunzip || !c->bgzf_ok || g_opt.no_device_inflate || !has_suffix(path, ".gz")) return 0;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return 0;
  struct stat st;
  mk_gzip_info info;
  if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || mk_gzip_scan_stream(fd, NULL, (size_t)st.st_size, &info) != MK_OK || !info.is_single) { close(fd); return 0; }
  mk_engine *e = sketch_engine(c);
  if (c->t_first_push == 0) c->t_first_push = now_s() - g_t0;
  mk_gunzip_stats gs;
  const int rc = c->occ ? mk_sketch_push_gzip_q(e, fd, (size_t)st.st_size, &g_opt.gunzip_opts, c->qmin, c->next_ordinal, &gs)
                        : mk_sketch_push_gzip(e, fd, (size_t)st.st_size, &g_opt.gunzip_opts, c->next_ordinal, &gs);
  close(fd);
  if (rc == MK_ERR_FORMAT) {
    drop_pushed_and_fall_back(c, e, gs.bad_status ? mk_gunzip_status_text(gs.bad_status) : "long line");
    return 0;
  }
  if (rc != MK_OK) die("%s failed (%d): %s", c->occ ? "mk_sketch_push_gzip_q" : "mk_sketch_push_gzip", rc, mk_bgzf_last_error());
  c->next_ordinal += gs.rows;
  c->nrows_total += gs.rows;
  c->t_last_push = now_s() - g_t0;
  if (g_opt.timing) {
    char members[96] = ""; /* --gunzip-members: how many the file had; --gunzip-repair: the piece starts it dropped */
    if (g_opt.gunzip_opts.flags & MK_GUNZIP_MEMBERS) snprintf(members, sizeof members, ", \"members\": %u", gs.members);
    if (g_opt.gunzip_opts.flags & MK_GUNZIP_REPAIR) {
      uint64_t repairs = 0;
      (void)mk_sketch_gunzip_repairs(e, &repairs);
      snprintf(members + strlen(members), sizeof members - strlen(members), ", \"repairs\": %llu", (unsigned long long)repairs);
    }
    printf("{\"input\": \"%s\", \"route\": \"device-gunzip\", \"pieces\": %llu, \"batches\": %llu, \"comp_bytes\": %llu, \"text_bytes\": %llu, \"rows\": %llu, "
           "\"find_ms\": %.3f, \"decode_ms\": %.3f, \"resolve_ms\": %.3f, \"frame_ms\": %.3f, \"read_s\": %.4f, \"route_total_s\": %.4f%s}\n",
           path, (unsigned long long)gs.pieces, (unsigned long long)gs.batches, (unsigned long long)gs.comp_bytes, (unsigned long long)gs.text_bytes,
           (unsigned long long)gs.rows, gs.find_ms, gs.decode_ms, gs.resolve_ms, gs.frame_ms, gs.t_read_s, gs.t_total_s, members);
  }
  return 1;
}
/* --long-reads: the file's text as it is, plain or through `zcat -fc`, in pieces of LONG_CHUNK bytes from two pinned
 * buffers in turn.  A push of pinned text returns once its copy and kernels are queued and is waited for at the start of the next
 * one, so buffer k ^ 1 is filled beside the copy and the kernels of buffer k -- two pieces in flight.  No framing on the host and
 * no limit on a line's length: the device keeps the sequence lines of complete records (mk_sketch_push_fastq_long). */
#define LONG_CHUNK ((size_t)32 << 20)
#define LONG_READERS 8
/* a plain file's next piece comes out of the page cache by several threads: one thread copies 8 GB/s, which alone bounded the route
 * at 0.52 s for 4 GB of text */
typedef struct { int fd; uint8_t *dst; off_t off; size_t n, got; } long_part;
static void *long_part_run(void *arg) {
  long_part *p = arg;
  while (p->got < p->n) {
    const ssize_t r = pread(p->fd, p->dst + p->got, p->n - p->got, p->off + (off_t)p->got);
    if (r <= 0) break;
    p->got += (size_t)r;
  }
  return NULL;
}
static size_t long_read_plain(int fd, uint8_t *dst, off_t off, size_t want, int nthreads) {
  long_part part[LONG_READERS];
  pthread_t th[LONG_READERS];
  int started[LONG_READERS];
  const int T = nthreads < 1 ? 1 : nthreads > LONG_READERS ? LONG_READERS : nthreads;
  const size_t per = ((want + (size_t)T - 1) / (size_t)T + 4095u) & ~(size_t)4095u;
  int np = 0;
  for (size_t at = 0; at < want; at += per, np++) {
    part[np] = (long_part){fd, dst + at, off + (off_t)at, want - at < per ? want - at : per, 0};
    started[np] = np > 0 && pthread_create(&th[np], NULL, long_part_run, &part[np]) == 0;
  }
  size_t have = 0;
  for (int i = 0; i < np; i++) {
    if (started[i]) pthread_join(th[i], NULL);
    else long_part_run(&part[i]); /* the first part, and any part whose thread did not start */
  }
  for (int i = 0; i < np; i++) { /* bytes in front of the first short part (the file ended there) */
    have += part[i].got;
    if (part[i].got < part[i].n) break;
  }
  return have;
}
static void report_long(const char *path, const char *route, unsigned long long pieces, unsigned long long bytes, double t_in) {
  if (!g_opt.timing) return;
  char fb[160] = "";
  if (g_gz_fallback) snprintf(fb, sizeof fb, ", \"fallback\": \"%s\"", g_gz_fallback);
  printf("{\"input\": \"%s\", \"route\": \"%s\", \"source\": \"%s\", \"pieces\": %llu, \"text_bytes\": %llu, \"route_total_s\": %.4f%s}\n", path,
         route, is_compressed(path) ? "zcat" : "file", pieces, bytes, now_s() - t_in, fb);
}
/* the long route of this file's reader: -A or -n / -Q (c->occ: fastq2co's rule with the -Q mask, 4.21) */
static const char *long_route(const ctx_t *c) { return c->occ ? "long-reads-q" : "long-reads"; }
static int long_push(const ctx_t *c, mk_engine *e, const uint8_t *text, uint64_t n, int final) {
  return c->occ ? mk_sketch_push_fastq_long_q(e, text, n, final, c->qmin) : mk_sketch_push_fastq_long(e, text, n, final);
}
static void sketch_fastq_long(ctx_t *c, const char *path) {
  for (int k = 0; k < 2; k++)
    if (!c->long_buf[k] && mk_host_alloc((void **)&c->long_buf[k], LONG_CHUNK) != MK_OK) die("out of memory");
  const double t_in = now_s();
  input_t in;
  if (!open_input(path, &in)) die("mtfastq2koc():%s: %s", path, strerror(errno));
  struct stat st;
  const int plain = in.pid == 0 && fstat(fileno(in.f), &st) == 0 && S_ISREG(st.st_mode);
  mk_engine *e = sketch_engine(c);
  if (c->t_first_push == 0) c->t_first_push = now_s() - g_t0;
  unsigned long long pieces = 0, bytes = 0;
  for (int k = 0;; k ^= 1) {
    repoison(c->long_buf[k], LONG_CHUNK);
    size_t have = 0, r;
    if (plain) have = long_read_plain(fileno(in.f), c->long_buf[k], (off_t)bytes, LONG_CHUNK, c->nthreads);
    else while (have < LONG_CHUNK && (r = fread(c->long_buf[k] + have, 1, LONG_CHUNK - have, in.f)) > 0) have += r;
    if (have == 0) break;
    CHECK(e, long_push(c, e, c->long_buf[k], have, 0));
    pieces++; bytes += have;
    if (have < LONG_CHUNK) break;
  }
  CHECK(e, long_push(c, e, NULL, 0, 1));
  /* --long-inflate: the device route had the file first and gave it up with a status.  The line then comes in front of the wait for
   * zcat, which may call the file damaged and end the run: why the file came this way is said either way */
  if (g_gz_fallback) report_long(path, long_route(c), pieces, bytes, t_in);
  close_input(&in);
  c->t_last_push = now_s() - g_t0;
  if (!g_gz_fallback) report_long(path, long_route(c), pieces, bytes, t_in);
}
/* --long-inflate: a .gz of the long-read route is inflated on the device and its text goes from HBM to the same framing.
 * A BGZF chain takes mk_sketch_push_bgzf_long, another file that mk_gzip_scan_stream calls single takes mk_sketch_push_gzip_long; 0:
 * neither, or the gzip route gave the file up with a status -- what was pushed is then finished and dropped and the caller reads the
 * file from its start through sketch_fastq_long (`zcat -fc`), which alone decides whether it is damaged.  A damaged BGZF block ends
 * the run with sketch_fastq_bgzf's message.  One file is one sketch here, so every call closes the stream (final). */
static int sketch_fastq_long_inflate(ctx_t *c, const char *path) {
  if (!(c->occ ? g_opt.long_inflate_q : g_opt.long_inflate) || !c->bgzf_ok || g_opt.no_device_inflate || !has_suffix(path, ".gz")) return 0;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return 0;
  struct stat st;
  if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size == 0) { close(fd); return 0; }
  const double t_in = now_s();
  mk_bgzf_block *tab = NULL;
  uint64_t nb = 0, total = 0;
  int is_bgzf = 0;
  if (mk_bgzf_scan(fd, NULL, (size_t)st.st_size, &tab, &nb, &total, &is_bgzf) == MK_OK && is_bgzf) {
    mk_bgzf_free(tab);
    mk_engine *e = sketch_engine(c);
    if (c->t_first_push == 0) c->t_first_push = now_s() - g_t0;
    mk_bgzf_opts o;
    memset(&o, 0, sizeof o);
    o.chunk_bytes = g_opt.inflate_chunk_bytes;
    mk_bgzf_stats bs;
    const int rc = c->occ ? mk_sketch_push_bgzf_long_q(e, fd, (size_t)st.st_size, &o, c->qmin, 1, &bs) : mk_sketch_push_bgzf_long(e, fd, (size_t)st.st_size, &o, 1, &bs);
    close(fd);
    if (rc == MK_ERR_FORMAT && bs.bad_block >= 0)
      die("%s: BGZF block %lld is damaged (%s): the input was not read completely", path, (long long)bs.bad_block, mk_inflate_status_text(bs.bad_status));
    if (rc != MK_OK) die("%s failed (%d): %s", c->occ ? "mk_sketch_push_bgzf_long_q" : "mk_sketch_push_bgzf_long", rc, mk_bgzf_last_error());
    c->t_last_push = now_s() - g_t0;
    if (g_opt.timing)
      printf("{\"input\": \"%s\", \"route\": \"%s\", \"source\": \"device-inflate\", \"blocks\": %llu, \"chunks\": %llu, \"comp_bytes\": %llu, "
             "\"text_bytes\": %llu, \"inflate_ms\": %.3f, \"frame_ms\": %.3f, \"bgzf_scan_s\": %.4f, \"read_s\": %.4f, \"route_total_s\": %.4f}\n",
             path, long_route(c), (unsigned long long)bs.blocks, (unsigned long long)bs.chunks, (unsigned long long)bs.comp_bytes, (unsigned long long)bs.text_bytes,
             bs.inflate_ms, bs.frame_ms, bs.t_scan_s, bs.t_read_s, now_s() - t_in);
    return 1;
  }
  mk_gzip_info info;
  if (mk_gzip_scan_stream(fd, NULL, (size_t)st.st_size, &info) != MK_OK || !info.is_single) { close(fd); return 0; }
  mk_engine *e = sketch_engine(c);
  if (c->t_first_push == 0) c->t_first_push = now_s() - g_t0;
  mk_gunzip_stats gs;
  const int rc = c->occ ? mk_sketch_push_gzip_long_q(e, fd, (size_t)st.st_size, &g_opt.gunzip_opts, c->qmin, 1, &gs)
                        : mk_sketch_push_gzip_long(e, fd, (size_t)st.st_size, &g_opt.gunzip_opts, 1, &gs);
  close(fd);
  if (rc == MK_ERR_FORMAT && gs.bad_status) {
    drop_pushed_and_fall_back(c, e, mk_gunzip_status_text(gs.bad_status));
    return 0;
  }
  if (rc != MK_OK) die("%s failed (%d): %s", c->occ ? "mk_sketch_push_gzip_long_q" : "mk_sketch_push_gzip_long", rc, mk_bgzf_last_error());
  c->t_last_push = now_s() - g_t0;
  if (g_opt.timing) {
    char members[96] = ""; /* --gunzip-members: how many the file had; --gunzip-repair: the piece starts it dropped */
    if (g_opt.gunzip_opts.flags & MK_GUNZIP_MEMBERS) snprintf(members, sizeof members, ", \"members\": %u", gs.members);
    if (g_opt.gunzip_opts.flags & MK_GUNZIP_REPAIR) {
      uint64_t repairs = 0;
      (void)mk_sketch_gunzip_repairs(e, &repairs);
      snprintf(members + strlen(members), sizeof members - strlen(members), ", \"repairs\": %llu", (unsigned long long)repairs);
    }
    printf("{\"input\": \"%s\", \"route\": \"%s\", \"source\": \"device-gunzip\", \"pieces\": %llu, \"batches\": %llu, \"comp_bytes\": %llu, "
           "\"text_bytes\": %llu, \"find_ms\": %.3f, \"decode_ms\": %.3f, \"resolve_ms\": %.3f, \"frame_ms\": %.3f, \"read_s\": %.4f, \"route_total_s\": %.4f%s}\n",
           path, long_route(c), (unsigned long long)gs.pieces, (unsigned long long)gs.batches, (unsigned long long)gs.comp_bytes, (unsigned long long)gs.text_bytes,
           gs.find_ms, gs.decode_ms, gs.resolve_ms, gs.frame_ms, gs.t_read_s, now_s() - t_in, members);
  }
  return 1;
}
static void sketch_fastq(ctx_t *c, const char *path) {
  if (c->occ ? g_opt.long_reads_q : g_opt.long_reads) {
    if (!sketch_fastq_long_inflate(c, path)) sketch_fastq_long(c, path);
    g_gz_fallback = NULL;
    return;
  }
  if (sketch_fastq_mapped(c, path)) return;
  if (sketch_fastq_bgzf(c, path)) return;
  if (sketch_fastq_gunzip(c, path)) return;
  if (is_compressed(path)) report_route(path, "zcat", NULL);
  g_gz_fallback = NULL;
  ensure_buffers(c);
  input_t in;
  if (!open_input(path, &in)) die("mtfastq2koc():%s: %s", path, strerror(errno));
  FILE *f = in.f;
  uint32_t stride = 160;
  size_t have = 0;
  int eof = 0;
  uint64_t records = 0;
  while (!eof || have) {
    if (!eof) {
      size_t r = fread(c->io + have, 1, IOBUF - have, f);
      have += r;
      if (r == 0) eof = 1;
    }
    size_t off = 0;
    for (;;) {
      uint64_t nrows = 0;
      size_t used = 0;
      uint64_t nrec = 0;
      /* every call starts at a record boundary (what is left of the buffer is moved to its front), which is what the
       * threaded framer needs */
      int rc = mk_fastq_frame_mt(c->io + off, have - off, eof, c->occ, c->qmin, c->TL, records, c->rows, stride, ROWBUF / stride,
                                 c->nthreads, &nrows, &nrec, &used);
      records += nrec;
      if (nrows) push_rows(c, c->rows, stride, nrows);
      off += used;
      if (rc == MK_ERR_ARG && stride < 4096) { stride = stride * 2 > 4096 ? 4096 : MK_ROW_PITCH(stride * 2); continue; } /* longer read: widen rows */
      if (rc == MK_ERR_ARG || rc == MK_ERR_FORMAT)
        die("%s: FASTQ line longer than the reference's fgets() width (%s): outside the framing contract", path,
            c->occ ? "19998 characters, iseq2comem.c:319,343" : "4094 characters, iseq2comem.c:656,673");
      if (rc != MK_OK) die("mk_fastq_frame failed (%d)", rc);
      if (nrows == 0 || off >= have) break;
    }
    memmove(c->io, c->io + off, have - off);
    have -= off;
    if (have == IOBUF) die("%s: a single FASTQ record exceeds the %zu-byte I/O buffer", path, IOBUF);
    if (eof && have && off == 0) break; /* trailing partial record: dropped like the reference does */
  }
  close_input(&in);
}
static void sketch_fasta(ctx_t *c, const char *path, int TL) {
  ensure_buffers(c);
  input_t in;
  if (!open_input(path, &in)) die("fasta2co():%s: %s", path, strerror(errno));
  FILE *f = in.f;
  if (!g_opt.host_fasta) {
    /* the file's bytes as they are, piece by piece: the device drops line ends and header lines (mk_sketch_push_stream) */
    mk_engine *e = sketch_engine(c);
    int any = 0;
    for (;;) {
      const size_t have = fread(c->io, 1, IOBUF, f);
      if (have == 0) break;
      any = 1;
      CHECK(e, mk_sketch_push_stream(e, c->io, have, 0));
    }
    if (!any) die("fastco():eof or fread error file=%s", path); /* iseq2comem.c:235 */
    CHECK(e, mk_sketch_push_stream(e, NULL, 0, 1));
    close_input(&in);
    return;
  }
  const uint32_t stride = MK_ROW_PITCH(512u); /* 528: not a multiple of 128 */
  mk_fasta_state st;
  if (mk_fasta_window_init(&st, TL) != MK_OK) die("mk_fasta_window_init failed");
  int eof = 0, any = 0;
  while (!eof) {
    size_t have = fread(c->io, 1, IOBUF, f);
    if (have == 0) eof = 1; else any = 1;
    size_t off = 0;
    do {
      uint64_t nrows = 0;
      size_t used = 0;
      const int wrc = mk_fasta_window(&st, c->io + off, have - off, eof, c->rows, stride, ROWBUF / stride, &nrows, &used);
      if (wrc == MK_ERR_FORMAT) die("fasta2co(): can not find seqences head start from '>' 0 (%s ends inside a header line)", path); /* iseq2comem.c:269 */
      if (wrc != MK_OK) die("mk_fasta_window failed (%d)", wrc);
      if (nrows) push_rows(c, c->rows, stride, nrows);
      off += used;
    } while (off < have);
  }
  if (!any) die("fastco():eof or fread error file=%s", path); /* iseq2comem.c:235 */
  close_input(&in);
}
/* ---- parallel front end for many small inputs (genome directories, many small FASTQ files) ---------------
 * The reference parallelises stage I over FILES (command_dist.c:363-366).  Here worker threads read and frame /
 * window whole files into pinned row buffers ahead of the main thread, which pushes and finishes them strictly
 * in input order (the order defines the sketch directory).  A file whose rows do not fit one buffer is left to
 * the main thread's streaming path.  Buffers are handed out in file order, so the pipeline cannot deadlock. */
#define PF_MAX_BUFS 16
typedef struct {
  int ready, too_big, err;   /* err: MK_ERR_* from framing */
  int buf;                   /* pinned buffer index, -1 = none */
  uint64_t nrows;
  uint32_t stride;
  uint64_t text_bytes;       /* FASTA for the device stream: the buffer holds the file's bytes, not rows */
  int is_text;
} pf_slot;
typedef struct {
  strlist *files;
  int TL;
  int qmin;      /* -Q (FASTQ without -A) */
  int koc_until; /* FASTQ files with an index below this are read the -A way (mt_shortreads2koc's reader), the others fastq2co's */
  int nbufs;
  uint8_t *bufs[PF_MAX_BUFS];
  int free_bufs[PF_MAX_BUFS], nfree;
  int next;                  /* next file index to prepare */
  pf_slot *slots;
  pthread_mutex_t mu;
  pthread_cond_t cv_buf, cv_ready;
} pf_t;
static uint8_t *slurp(const char *path, size_t *n_out, size_t limit, int *too_big) {
  input_t in;
  if (!open_input(path, &in)) return NULL;
  size_t cap = (size_t)8 << 20, n = 0;
  uint8_t *b = malloc(cap);
  if (!b) die("out of memory");
  for (;;) {
    if (n == cap) {
      if (cap >= limit) { *too_big = 1; break; }
      cap *= 2;
      uint8_t *nb = realloc(b, cap);
      if (!nb) die("out of memory");
      b = nb;
    }
    size_t r = fread(b + n, 1, cap - n, in.f);
    if (r == 0) break;
    n += r;
  }
  if (*too_big && in.pid > 0) { /* the rest is read again by the streaming path: do not wait for zcat to push it all out */
    fclose(in.f); in.f = NULL;
    kill(in.pid, SIGTERM);
    waitpid(in.pid, NULL, 0);
  } else close_input(&in);
  *n_out = n;
  return b;
}
/* the bytes of an uncompressed regular file straight into `dst` (a pinned row buffer): 1 = done, 0 = not that kind of file or
 * larger than cap */
static int slurp_into(const char *path, uint8_t *dst, size_t cap, size_t *n_out) {
  if (is_compressed(path)) return 0;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return 0;
  struct stat st;
  if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || (size_t)st.st_size > cap) { close(fd); return 0; }
  size_t n = 0;
  while (n < (size_t)st.st_size) {
    const ssize_t r = read(fd, dst + n, (size_t)st.st_size - n);
    if (r <= 0) break;
    n += (size_t)r;
  }
  close(fd);
  if (n != (size_t)st.st_size) return 0;
  *n_out = n;
  return 1;
}
static void *pf_worker(void *arg) {
  pf_t *pf = arg;
  for (;;) {
    pthread_mutex_lock(&pf->mu);
    while (pf->next < pf->files->n && pf->nfree == 0) pthread_cond_wait(&pf->cv_buf, &pf->mu);
    if (pf->next >= pf->files->n) { pthread_mutex_unlock(&pf->mu); return NULL; }
    const int i = pf->next++;
    const int b = pf->free_bufs[--pf->nfree];
    pthread_mutex_unlock(&pf->mu);
    repoison(pf->bufs[b], ROWBUF);

    pf_slot s = {0};
    s.buf = b;
    const char *path = pf->files->v[i];
    size_t n = 0;
    int too_big = 0;
    if (!g_opt.host_fasta && !is_fastq(path)) {
      /* FASTA for the device stream: the file's bytes go into the pinned buffer as they are (no parsing on the host) */
      if (slurp_into(path, pf->bufs[b], ROWBUF, &n)) {
        if (n == 0) s.err = MK_ERR_STATE; /* empty input: the reference's "eof or fread error" (iseq2comem.c:235) */
        s.is_text = 1; s.text_bytes = n;
        pthread_mutex_lock(&pf->mu);
        if (s.err) { pf->free_bufs[pf->nfree++] = b; s.buf = -1; pthread_cond_broadcast(&pf->cv_buf); }
        s.ready = 1;
        pf->slots[i] = s;
        pthread_cond_broadcast(&pf->cv_ready);
        pthread_mutex_unlock(&pf->mu);
        continue;
      }
      /* compressed, a pipe, or larger than a buffer: through a heap copy below */
    }
    uint8_t *text = slurp(path, &n, ROWBUF, &too_big);
    if (!text) s.err = MK_ERR_IO;
    else if (too_big) s.too_big = 1;
    else if (is_fastq(path)) {
      uint32_t stride = 160;
      for (;;) {
        uint64_t nrows = 0;
        size_t used = 0;
        uint64_t nrec = 0;
        int rc = i >= pf->koc_until ? mk_fastq_frame_q(text, n, 1, pf->qmin, pf->TL, 0, pf->bufs[b], stride, ROWBUF / stride, &nrows, &nrec, &used)
                                    : mk_fastq_frame(text, n, 1, pf->bufs[b], stride, ROWBUF / stride, &nrows, &used);
        if (rc == MK_ERR_ARG && stride < 4096) { stride = stride * 2 > 4096 ? 4096 : MK_ROW_PITCH(stride * 2); continue; }
        if (rc != MK_OK) s.err = rc;
        else if (used < n) s.too_big = 1; /* more rows than one buffer holds */
        s.nrows = nrows; s.stride = stride;
        break;
      }
    } else if (!g_opt.host_fasta) {
      if (n == 0) s.err = MK_ERR_STATE;
      else { memcpy(pf->bufs[b], text, n); s.is_text = 1; s.text_bytes = n; } /* (.gz genomes: the text came through zcat) */
    } else {
      mk_fasta_state st;
      const uint32_t stride = MK_ROW_PITCH(512u); /* 528: not a multiple of 128 */
      uint64_t nrows = 0;
      size_t used = 0;
      if (n == 0) s.err = MK_ERR_STATE; /* empty input: the reference's "eof or fread error" (iseq2comem.c:235) */
      else {
        mk_fasta_window_init(&st, pf->TL);
        int rc = mk_fasta_window(&st, text, n, 1, pf->bufs[b], stride, ROWBUF / stride, &nrows, &used);
        if (rc != MK_OK) s.err = rc;
        else if (used < n || st.fresh) s.too_big = 1;
        s.nrows = nrows; s.stride = stride;
      }
    }
    free(text);
    pthread_mutex_lock(&pf->mu);
    if (s.too_big || s.err) { pf->free_bufs[pf->nfree++] = b; s.buf = -1; pthread_cond_broadcast(&pf->cv_buf); }
    s.ready = 1;
    pf->slots[i] = s;
    pthread_cond_broadcast(&pf->cv_ready);
    pthread_mutex_unlock(&pf->mu);
  }
}
/* ---- one input file -> one sketch on the engine(s) of `c` (run_stageI()'s loop body, command_dist.c:367-404) ------------- */
typedef struct {
  strlist *files;
  const mk_params *P;
  int abundance, uniq, first_nonfq, kmerocrs, kmerqlty, nthreads, quiet;
  pf_t *pf;
  int nworkers;
} job_opts;
/* first half: begin + everything pushed (queued on the engine's stream: a pinned text buffer stays with the caller in *held
 * until the finish has waited); second half: finish + the reference's error messages */
static void sketch_file_push(ctx_t *c, const job_opts *o, int i, int *held_out) {
  const char *path = o->files->v[i];
  c->next_ordinal = 0;
  const int fq = is_fastq(path);
  /* -A holds until the file loop reaches the first input that is no FASTQ (command_dist.c:389-392) */
  const int abundance = o->abundance && i < o->first_nonfq;
  if (fq && abundance && !o->quiet) printf("running mt_shortreads2koc()\n");
  c->begun = 0;
  c->mode = fq ? (abundance ? MK_MODE_KOC : MK_MODE_OCC_SET) : (o->uniq ? MK_MODE_UNIQ_SET : MK_MODE_SET);
  c->min_occ = o->kmerocrs;
  c->occ = fq && !abundance; c->qmin = o->kmerqlty; c->TL = o->P->TL; c->nthreads = o->nthreads;
  int handled = 0, held = -1;
  pf_t *pf = o->pf;
  if (!fq && is_compressed(path)) report_route(path, "zcat", NULL); /* (a FASTQ input says so where its reader is chosen) */
  if (o->nworkers) {
    pthread_mutex_lock(&pf->mu);
    while (!pf->slots[i].ready) pthread_cond_wait(&pf->cv_ready, &pf->mu);
    pf_slot sl = pf->slots[i];
    pthread_mutex_unlock(&pf->mu);
    if (sl.err == MK_ERR_IO) die("%s: cannot open", path);
    if (sl.err == MK_ERR_STATE && !fq) die("fastco():eof or fread error file=%s", path);
    if (sl.err == MK_ERR_FORMAT && !fq) die("fasta2co(): can not find seqences head start from '>' 0 (%s ends inside a header line)", path);
    if (sl.err) die("%s: sequence or header line of 4095+ characters: outside the FASTQ framing contract (iseq2comem.c:656,673)", path);
    if (!sl.too_big) {
      if (sl.is_text) {
        mk_engine *e = sketch_engine(c);
        CHECK(e, mk_sketch_push_stream(e, pf->bufs[sl.buf], sl.text_bytes, 1));
        held = sl.buf; /* pinned text: the copy is queued, the buffer goes back once the finish below has waited */
      } else {
        if (sl.nrows) push_rows(c, pf->bufs[sl.buf], sl.stride, sl.nrows);
        pthread_mutex_lock(&pf->mu); /* push returned: the buffer has been copied to the device */
        pf->free_bufs[pf->nfree++] = sl.buf;
        pthread_cond_broadcast(&pf->cv_buf);
        pthread_mutex_unlock(&pf->mu);
      }
      handled = 1;
    }
  }
  if (!handled) {
    if (fq) sketch_fastq(c, path);
    else sketch_fasta(c, path, o->P->TL);
  }
  (void)sketch_engine(c); /* an input without a single row still gives an (empty) sketch */
  *held_out = held;
}
static void sketch_file_finish(ctx_t *c, const job_opts *o, int i, int held, mk_result *res, double *t_finish) {
  const char *path = o->files->v[i];
  pf_t *pf = o->pf;
  mk_engine *eng = c->eng;
  const double tf = now_s();
  int rc;
  if (c->multi) {
    rc = g_multi.finish(c->multi, res, &c->gather_ms, &c->tail_ms);
    if (rc != MK_OK && rc != MK_ERR_CROWDED) die("mk_multi_finish failed (%d): %s", rc, g_multi.last_error(c->multi));
  } else if (c->want_keys) rc = mk_sketch_finish_keys(eng, &c->keys, &c->kcnt, &c->nkeys);
  else rc = mk_sketch_finish(eng, res);
  *t_finish += now_s() - tf;
  if (held >= 0) {
    pthread_mutex_lock(&pf->mu);
    pf->free_bufs[pf->nfree++] = held;
    pthread_cond_broadcast(&pf->cv_buf);
    pthread_mutex_unlock(&pf->mu);
  }
  if (rc == MK_ERR_CROWDED) die("the context space is too crowd, try rerun the program using -k%d", o->P->k + 1);
  if (rc == MK_ERR_FORMAT) die("fasta2co(): can not find seqences head start from '>' 0 (%s ends inside a header line)", path); /* iseq2comem.c:269 */
  if (rc != MK_OK) die("mk_sketch_finish failed (%d): %s", rc, mk_last_error(eng));
}
static int sketch_one_file(ctx_t *c, const job_opts *o, int i, mk_result *res, double *t_finish) {
  int held = -1;
  sketch_file_push(c, o, i, &held);
  sketch_file_finish(c, o, i, held, res, t_finish);
  return MK_OK;
}
/* ---- several GPUs, several files: whole files are the unit (SURVEY.md 8e "config 5"; the reference's team over files,
 * command_dist.c:363-372).  One engine and one driver thread per listed GPU; the drivers take the next file from a shared
 * cursor, sketch it whole on their engine and leave a copy of the result; the main thread writes the results in file order.
 * No exchange between GPUs, no RCCL.  Naming one GPU several times gives that many engines on it: one file's finish then runs
 * beside the next file's scan. */
typedef struct {
  int ready;
  mk_result res;       /* a copy: components, ids and counts in malloc'ed memory */
} file_result;
typedef struct {
  pthread_t th;
  ctx_t c;
  engine_future fut_dummy;
  const job_opts *o;
  int device;
  int *cursor;
  file_result *out;
  pthread_mutex_t *mu;
  pthread_cond_t *cv;
  double t_finish;
  int created;
} shard_driver;
static void copy_result(const mk_result *r, mk_result *dst) {
  dst->component_num = r->component_num;
  dst->total = r->total;
  dst->components = malloc(sizeof(mk_component) * (size_t)(r->component_num > 0 ? r->component_num : 1));
  if (!dst->components) die("out of memory");
  for (int k = 0; k < r->component_num; k++) {
    const mk_component *a = &r->components[k];
    mk_component *b = &dst->components[k];
    b->n = a->n;
    b->ids = a->n ? malloc(4 * (size_t)a->n) : NULL;
    b->counts = a->n && a->counts ? malloc(2 * (size_t)a->n) : NULL;
    if (a->n && (!b->ids || (a->counts && !b->counts))) die("out of memory");
    if (a->n) memcpy(b->ids, a->ids, 4 * (size_t)a->n);
    if (a->n && a->counts) memcpy(b->counts, a->counts, 2 * (size_t)a->n);
  }
}
static void free_result(mk_result *r) {
  for (int k = 0; k < r->component_num; k++) { free(r->components[k].ids); free(r->components[k].counts); }
  free(r->components);
  r->components = NULL;
}
static void *shard_driver_run(void *arg) {
  shard_driver *d = arg;
  if (!d->c.eng) { /* engines 1..: created here, all at the same time; engine 0 came through the start-up future */
    mk_engine *e = NULL;
    const int rc = mk_engine_create(d->o->P, d->device, &e);
    if (rc != MK_OK) die("mk_engine_create on GPU %d failed (%d): %s", d->device, rc, mk_last_error(NULL));
    d->c.eng = e;
    d->c.engs[0] = e;
    engine_apply_options(&d->c, e);
  }
  for (;;) {
    pthread_mutex_lock(d->mu);
    const int i = (*d->cursor)++;
    pthread_mutex_unlock(d->mu);
    if (i >= d->o->files->n) return NULL;
    mk_result res;
    sketch_one_file(&d->c, d->o, i, &res, &d->t_finish);
    file_result fr;
    memset(&fr, 0, sizeof fr);
    copy_result(&res, &fr.res);
    mk_result_release(d->c.eng, &res);
    fr.ready = 1;
    pthread_mutex_lock(d->mu);
    d->out[i] = fr;
    pthread_cond_broadcast(d->cv);
    pthread_mutex_unlock(d->mu);
  }
}
/* engines beside the first one on the same GPU, created one after the other by a thread of their own; `ready` counts them */
#define MAX_ENGINES_PER_GPU 4
typedef struct { pthread_t th; const mk_params *P; int device, want; mk_engine *eng[MAX_ENGINES_PER_GPU - 1]; int ready, failed; char err[512]; } extra_engines_t;
static void *extra_engines_run(void *arg) {
  extra_engines_t *s = arg;
  for (int k = 0; k < s->want; k++) {
    if (mk_engine_create(s->P, s->device, &s->eng[k]) != MK_OK) {
      s->eng[k] = NULL;
      snprintf(s->err, sizeof s->err, "%s", mk_last_error(NULL));
      __atomic_store_n(&s->failed, 1, __ATOMIC_RELEASE);
      break;
    }
    __atomic_store_n(&s->ready, k + 1, __ATOMIC_RELEASE);
  }
  return NULL;
}
/* ---- a directory of genomes in batches (mk_sketch_batch_begin / _end) -------------------------------------------------------
 * The reference sketches one file per OpenMP thread (command_dist.c:363-372).  Here consecutive small FASTA files go to the
 * device TOGETHER: the reader threads do the FASTA walk and leave the files of a batch as PACKED ROWS in one pinned buffer
 * (mk_fasta_pack_rows; the scan kernel reads them there), the engine runs ONE launch sequence for all of them, and two batches are
 * in flight while the readers fill the next.  (--batch-text, and every geometry without a scan kernel for packed rows: the files'
 * TEXT at 1 KiB-aligned offsets, one host-to-device copy, the walk on the device.)
 * A file that cannot go that way (FASTQ, compressed, a pipe, larger than BATCH_FILE_MAX) is sketched alone, in its place in the
 * input order.  --no-batch gives the file-by-file driver. */
#define BATCH_FILE_MAX ((size_t)32 << 20)
#define BATCH_BUFS 4      /* buffers of text batches; packed rows: as many as 2 GiB hold, BATCH_BUFS_MAX at most */
#define BATCH_BUFS_MAX 64

typedef struct { int first, n, batch, gz, nsub; } bjob; /* files [first, first + n); batch: its number among the batches, -1 = one file alone;
                                                         * gz: single-member gzip files, inflated on the device; nsub: files the engine got */
typedef struct {
  strlist *files;
  uint64_t *fsize;              /* per file: size when the batches were planned; a reader that meets EOF earlier writes what it got */
  uint8_t *grew;                /* per file: there are bytes behind that size -- the file is sketched alone, from all of its text */
  const uint8_t *kind;          /* per file: 1 plain text, 2 a gzip file whose BYTES travel (its place holds them as they are) */
  bjob *jobs; int njobs;
  uint8_t *buf[BATCH_BUFS_MAX]; size_t bufcap; int nbufs;
  uint64_t *foff;               /* offset of every file inside its batch's buffer */
  uint32_t rows_format;         /* MK_ROWS_PACKED / MK_ROWS_WIDE */
  int rows_TL;                  /* != 0: the readers do the FASTA walk and leave PACKED ROWS in the buffer (mk_fasta_pack_rows) ... */
  uint64_t *slot_rows, *nrows;  /* ... per file: rows its place in the buffer holds / rows it got */
  uint8_t **priv;               /* ... per file: rows that did not fit its place (wide rows: more extension rows than the place allows for) */
  int *left;                    /* per job: files not read yet */
  int *failed;                  /* per file: errno of a failed read */
  int released;                 /* batches whose buffer has been handed back */
  double cpu_read, cpu_pack, cpu_blocked; /* summed over the readers: seconds in pread(), in mk_fasta_pack_rows(), waiting for a free buffer */
  int next_job, next_file;      /* reader cursor */
  pthread_mutex_t mu;
  pthread_cond_t cv_ready, cv_free;
} breader;
static void *breader_run(void *arg) {
  breader *r = arg;
  uint8_t *txt = NULL; /* rows: the file's text, here only */
  size_t txt_cap = 0;
  for (;;) {
    pthread_mutex_lock(&r->mu);
    while (r->next_job < r->njobs && (r->jobs[r->next_job].batch < 0 || r->next_file >= r->jobs[r->next_job].n)) { r->next_job++; r->next_file = 0; }
    if (r->next_job >= r->njobs) { pthread_mutex_unlock(&r->mu); free(txt); return NULL; }
    const int j = r->next_job, k = r->next_file++;
    const bjob *job = &r->jobs[j];
    const double tb0 = now_s();
    while (job->batch - r->released >= r->nbufs) pthread_cond_wait(&r->cv_free, &r->mu); /* its buffer still belongs to an older batch */
    r->cpu_blocked += now_s() - tb0;
    pthread_mutex_unlock(&r->mu);
    const double tr0 = now_s();
    double tr1 = tr0;
    const int i = job->first + k;
    uint8_t *const place = r->buf[job->batch % r->nbufs] + r->foff[i];
    uint8_t *dst = place;
    int err = 0;
    const int rows_TL = r->kind[i] == 2 ? 0 : r->rows_TL;
    if (rows_TL) {
      if (txt_cap < r->fsize[i] + 64) {
        free(txt);
        txt_cap = (size_t)r->fsize[i] + ((size_t)1 << 20);
        txt = malloc(txt_cap);
        if (!txt) { txt_cap = 0; err = ENOMEM; }
      }
      dst = txt;
    }
    const int fd = err ? -1 : open(r->files->v[i], O_RDONLY);
    if (err) ;
    else if (fd < 0) err = errno ? errno : EIO;
    else {
      /* to EOF, like the reference and the file-by-file driver (zcat -fc | fread: iseq2comem.c:226-233), within the file's place:
       * a file that SHRANK since the batches were planned is what it is now; one that GREW cannot travel in its place and is
       * sketched alone (the batch carries its first bytes along, their result is dropped) */
      uint64_t got = 0;
      while (got < r->fsize[i]) {
        const ssize_t n = pread(fd, dst + got, (size_t)(r->fsize[i] - got), (off_t)got);
        if (n < 0) { if (errno == EINTR) continue; err = errno ? errno : EIO; break; }
        if (n == 0) break;
        got += (uint64_t)n;
      }
      if (!err) {
        uint8_t probe;
        if (got < r->fsize[i]) r->fsize[i] = got;
        else if (pread(fd, &probe, 1, (off_t)got) > 0) { r->grew[i] = 1; r->fsize[i] = 0; } /* an empty member of its batch */
      }
      close(fd);
    }
    tr1 = now_s();
    if (rows_TL && !err && r->grew[i]) r->nrows[i] = 0;
    else if (rows_TL && !err) {
      /* the walk and the packing here, on this thread (what the file leaves free of its place is never looked at) */
      uint64_t got_rows = 0;
      int prc = mk_fasta_pack_rows(txt, (size_t)r->fsize[i], rows_TL, r->rows_format, place, r->slot_rows[i], &got_rows);
      if (prc == MK_ERR_ARG) { /* more rows than its place holds: into memory of its own (the batch's rows are then copied to the device) */
        const uint64_t full = mk_fasta_pack_bound((size_t)r->fsize[i], rows_TL, r->rows_format);
        void *own = NULL;
        if (posix_memalign(&own, 64, (size_t)(full ? full : 1) * MK_PACKED_PITCH) != 0) { prc = MK_ERR_NOMEM; }
        else {
          prc = mk_fasta_pack_rows(txt, (size_t)r->fsize[i], rows_TL, r->rows_format, own, full, &got_rows);
          if (prc == MK_OK) r->priv[i] = own; else free(own);
        }
      }
      if (prc == MK_ERR_FORMAT) err = -MK_ERR_FORMAT + 100000; /* (no errno: the text ends inside a '>' line) */
      else if (prc != MK_OK) err = EIO;
      else r->nrows[i] = got_rows;
    }
    pthread_mutex_lock(&r->mu);
    r->cpu_read += tr1 - tr0; r->cpu_pack += now_s() - tr1;
    r->failed[i] = err;
    if (--r->left[j] == 0) pthread_cond_broadcast(&r->cv_ready);
    pthread_mutex_unlock(&r->mu);
  }
}
/* ---- the stage-I driver ------------------------------------------------------------------------------------------------------ */
#ifndef MK_DEFAULT_ENGINES
#define MK_DEFAULT_ENGINES 2
#endif
/* dist -A --composite: the marker database is loaded by a thread of its own while the first file is read; every
 * sample's key list then goes from the engine to the handle on the device, and a batch is flushed through the report when it holds
 * batch_limit bytes of ids and at the end */
typedef struct {
  pthread_t th;
  int on, joined, device, rhave;
  const char *refdir, *abv_dir;
  costat rs;
  mk_composite *h;
  composite_vec *vec;
  uint64_t *row_end;
  int batch_first, batch_n; /* the open batch: its first file, its samples so far */
  uint64_t batch_ids_bytes, batch_limit, batches, hits;
  double load_ms, query_ms;
} fused_t;
static void *fused_load_run(void *arg) { /* as composite_resident() loads it (cli_composite.c) */
  fused_t *f = arg;
  const int ref_n = f->rs.infile_num, comp_num = f->rs.comp_num;
  if (mk_composite_create(f->device, &f->h) != MK_OK) die("mk_composite_create failed: %s", mk_composite_last_error(NULL));
  if (mk_composite_load_begin(f->h, (uint32_t)ref_n, (uint32_t)comp_num) != MK_OK) die("get_species_abundance(): %s", mk_composite_last_error(f->h));
  for (int c = 0; c < comp_num; c++) {
    size_t n1, n2;
    uint8_t *rco = need_part("get_species_abundance():", f->refdir, "combco", c, 0, &n1);
    uint8_t *ridx = need_part("get_species_abundance():", f->refdir, "combco.index", c, 8 * ((size_t)ref_n + 1), &n2);
    if (((const uint64_t *)ridx)[ref_n] * 4 > n1) die("get_species_abundance(): component %d is shorter than its index says", c);
    if (mk_composite_load_component(f->h, (uint32_t)c, (const uint32_t *)rco, (const uint64_t *)ridx) != MK_OK)
      die("get_species_abundance(): %s", mk_composite_last_error(f->h));
    free(rco); free(ridx);
  }
  return NULL;
}
/* what one run of stage I carries from the plan through one of the four file loops to the --timing line */
typedef struct {
  strlist files; mk_shuf sh; mk_params P; mk_sketchdir *sd; fused_t fu;
  job_opts jo; ctx_t c; engine_future fut; pf_t pf; extra_engines_t extra;
  int quiet, stage2_after, shard_files, use_batch, n_engines, nthreads, nbatches_done;
  int done_files;     /* the batch loop's progress count */
  uint64_t *fsize;    /* the plan, per file: its size when the batches were planned, */
  uint8_t *elig;      /* 1: plain text; 2: a single-member gzip file (mk_gzip_scan), inflated on the device, */
  uint32_t *gz_isize; /* and a gzip file's text size */
  uint64_t gun_S, gun_R; /* S and R of the --device-gunzip route as the library will clamp them */
  double t_shuf, t_written, t_finish, t_batch_wait_read, t_batch_pin, t_batch_begin, t_readers_read, t_readers_pack, t_readers_blocked;
} stage1;
/* the batch loop's state: the readers' (jobs, fsize, grew, foff, left, failed, slot_rows, nrows, priv, buf, bufcap, nbufs) and what
 * is handed to the engine */
typedef struct {
  stage1 *s; breader br; int nbatches, batch_rows;
  int *gzpos; /* a gzip file's index in the batch the engine got, -1: it does not travel in it */
  mk_batch_file *bf; mk_batch_result *bres; mk_gz_file *gzf; uint32_t *gzst, *gzpc;
  int buf_pinned[BATCH_BUFS_MAX], fly[2], nfly, btrace;
} batch_run;
/* one file's sketch into the directory (the files come in input order) and its progress line; `owner` takes the result back, NULL:
 * it is a copy or goes with its batch */
static void emit_result(stage1 *s, int file, mk_engine *owner, mk_result *res) {
  const char *path = s->files.v[file];
  const int rc = mk_sketchdir_add(s->sd, path, res);
  if (rc != MK_OK) die("writing sketch for %s failed (%d)", path, rc);
  if (owner) mk_result_release(owner, res);
  if (!s->quiet) printf("%d/%d decomposing %s\r", s->use_batch ? ++s->done_files : file + 1, s->files.n, path);
}
/* the open batch through the report: the lines (or .abv files) of its samples, in file order */
static void fused_flush(stage1 *s) {
  fused_t *f = &s->fu;
  if (!f->batch_n) return;
  const mk_composite_row *rows = NULL;
  if (mk_composite_query_finish(f->h, &rows, f->row_end) != MK_OK) die("get_species_abundance(): %s", mk_composite_last_error(f->h));
  for (int k = 0; k < f->batch_n; k++) {
    const uint64_t lo = k ? f->row_end[k - 1] : 0;
    composite_write_sample(rows + lo, f->row_end[k] - lo, s->files.v[f->batch_first + k], f->rs.names, f->refdir, f->abv_dir, g_opt.abv, f->vec);
  }
  uint64_t bh = 0, br = 0;
  double lm = 0.0, qm = 0.0;
  mk_composite_last_counts(f->h, &bh, &br);
  mk_composite_last_kernel_ms(f->h, &lm, &qm);
  f->hits += bh; f->query_ms += qm; f->load_ms = lm;
  f->batches++;
  f->batch_n = 0; f->batch_ids_bytes = 0;
}
/* the file's sketch has ended at the engine's key list (ctx_t::keys): it becomes the next sample of the open batch.  The batch is
 * begun with room for every file still to come; it is finished as soon as it holds batch_limit bytes of ids (the samples that have
 * not come by then are empty and print nothing) */
static void fused_sample(stage1 *s, int file) {
  fused_t *f = &s->fu;
  const ctx_t *c = &s->c;
  if (!f->joined) { pthread_join(f->th, NULL); f->joined = 1; }
  if (!f->batch_n) {
    if (mk_composite_query_begin(f->h, (uint32_t)(s->files.n - file)) != MK_OK) die("get_species_abundance(): %s", mk_composite_last_error(f->h));
    f->batch_first = file;
  }
  if (mk_composite_query_sample_keys(f->h, (uint32_t)f->batch_n, c->keys, c->kcnt, c->nkeys, (uint32_t)s->P.comp_code_bits) != MK_OK)
    die("get_species_abundance(): %s", mk_composite_last_error(f->h));
  f->batch_n++;
  f->batch_ids_bytes += c->nkeys * 4;
  if (f->batch_ids_bytes >= f->batch_limit || file + 1 == s->files.n) fused_flush(s);
}
static void sketch_and_emit(stage1 *s, int file) { /* one file alone on the first engine */
  mk_result res;
  sketch_one_file(&s->c, &s->jo, file, &res, &s->t_finish);
  if (s->fu.on) fused_sample(s, file);
  else emit_result(s, file, s->c.eng, &res);
}
/* which inputs can travel in batches: plain FASTA files of moderate size, when the device parses the text and one engine works;
 * then (two of them at least) the jobs in input order: runs of eligible files cut into batches, every other file alone */
static void plan_batches(stage1 *s, batch_run *b) {
  cli_opts *o = &g_opt; /* (batch_bytes is settled here) */
  const strlist *files = &s->files; const mk_params *P = &s->P;
  uint64_t *fsize = s->fsize = calloc((size_t)files->n, sizeof *fsize);
  uint8_t *elig = s->elig = calloc((size_t)files->n, 1);
  uint32_t *gz_isize = s->gz_isize = calloc((size_t)files->n, sizeof *gz_isize);
  if (!fsize || !elig || !gz_isize) die("out of memory");
  if (files->n <= 1 || o->no_batch || o->host_fasta || o->engines_per_gpu || s->shard_files || o->ndev > 1 || o->composite_db) return;
  const uint64_t gun_S = s->gun_S, gun_R = s->gun_R;
  int n_elig = 0;
  if (o->batch_files < 1 || o->batch_files > (int)MK_BATCH_MAX_FILES) die("--batch-files takes 1..%u", MK_BATCH_MAX_FILES);
  /* a batch's tables hold about five times the keys its files are expected to leave (text / 16^drlevel), 2^26 slots at most */
  const size_t geo_cap = (((size_t)1 << 25) / 5u) << (4 * P->drlevel > 20 ? 20 : 4 * P->drlevel);
  /* rows, small sketches (drlevel >= 3: a key in 4 096 k-mers): 256 MiB of text a batch -- the kernels behind a batch's scan (tables,
   * layout, dump: 0.15-0.2 ms during which the link idles) come half as often as with 128 MiB: 1 024 genomes 3 ms sooner at L3K10.
   * Larger sketches (L2K11: a key in 256) keep 128 MiB: their tables and dumps grow with the batch, 256 MiB was 0-5 ms slower there,
   * 512 MiB 15 ms */
  if (!o->batch_bytes) o->batch_bytes = (!o->batch_text && mk_params_packed_ok(P) && P->drlevel >= 3) ? (size_t)256 << 20 : (size_t)128 << 20;
  if (o->batch_bytes > geo_cap) o->batch_bytes = geo_cap;
  if (o->batch_bytes > ((size_t)512 << 20)) o->batch_bytes = (size_t)512 << 20;
  if (o->batch_bytes < ((size_t)1 << 20)) o->batch_bytes = (size_t)1 << 20;
  for (int i = 0; i < files->n; i++) {
    struct stat fst;
    if (is_fastq(files->v[i]) || stat(files->v[i], &fst) != 0 || !S_ISREG(fst.st_mode)) continue;
    if (fst.st_size <= 0 || (size_t)fst.st_size > BATCH_FILE_MAX || (size_t)fst.st_size > o->batch_bytes) continue;
    if (is_compressed(files->v[i])) { /* what genome archives ship: one gzip member.  Anything else keeps the zcat route */
      if (!o->gz_batches || !has_suffix(files->v[i], ".gz")) continue;
      const int fd = open(files->v[i], O_RDONLY);
      if (fd < 0) continue;
      mk_gzip_info gi;
      const int grc = mk_gzip_scan(fd, NULL, (size_t)fst.st_size, &gi);
      close(fd);
      if (grc != MK_OK || !gi.is_single || gi.isize > BATCH_FILE_MAX || gi.isize > o->batch_bytes) continue;
      if (o->gz_gunzip && ((gi.pay_len + gun_S - 1) / gun_S > MK_GUNZIP_BATCH_SPANS_MAX || (gi.pay_len + (gi.pay_len + gun_S - 1) / gun_S) * gun_R > MK_GUNZIP_BATCH_SYMS_MAX))
        continue; /* (too large for a batch of its own at this span and ratio) */
      fsize[i] = (uint64_t)fst.st_size; gz_isize[i] = gi.isize; elig[i] = 2; n_elig++;
      continue;
    }
    fsize[i] = (uint64_t)fst.st_size; elig[i] = 1; n_elig++;
  }
  /* test hook (tests/test_golden.py): MK_TEST_PLAN_SKEW="<m>:<d>" plans every m-th file with a size off by d bytes, i.e. as if
   * the file had grown (d < 0) or shrunk (d > 0) between this stat() and the readers' pread() */
  if (getenv("MK_TEST_PLAN_SKEW")) {
    int m = 0; long d = 0;
    if (sscanf(getenv("MK_TEST_PLAN_SKEW"), "%d:%ld", &m, &d) == 2 && m > 0)
      for (int i = 0; i < files->n; i += m)
        if (elig[i] && (d > 0 || fsize[i] > (uint64_t)(-d))) fsize[i] = (uint64_t)((long)fsize[i] + d);
  }
  s->use_batch = n_elig >= 2;
  if (!s->use_batch) return;

  breader *br = &b->br;
  b->s = s;
  bjob *jobs = br->jobs = calloc((size_t)files->n, sizeof *jobs);
  uint64_t *foff = br->foff = calloc((size_t)files->n, sizeof *foff);
  br->left = calloc((size_t)files->n, sizeof *br->left); br->failed = calloc((size_t)files->n, sizeof *br->failed);
  br->grew = calloc((size_t)files->n + 1, 1);
  /* the readers do the FASTA walk and pack (0.48 bytes a base cross PCIe instead of 1.01, and the scan kernel reads them where the
   * readers left them) wherever there is a scan kernel for packed rows; --batch-text: the text travels and the device walks it */
  const int batch_rows = b->batch_rows = !o->batch_text && mk_params_packed_ok(P);
  const uint32_t rows_format = o->batch_narrow ? MK_ROWS_PACKED : MK_ROWS_WIDE;
  uint64_t *slot_rows = br->slot_rows = calloc((size_t)files->n, sizeof *slot_rows);
  br->nrows = calloc((size_t)files->n, sizeof *br->nrows);
  br->priv = calloc((size_t)files->n, sizeof *br->priv);
  b->gzpos = calloc((size_t)files->n, sizeof *b->gzpos);
  if (!jobs || !foff || !br->left || !br->failed || !slot_rows || !br->nrows || !br->priv || !br->grew || !b->gzpos) die("out of memory");
  int njobs = 0, nbatches = 0;
  size_t bufcap = 0;
  for (int i = 0; i < files->n;) {
    if (!elig[i]) { jobs[njobs].first = i; jobs[njobs].n = 1; jobs[njobs].batch = -1; njobs++; i++; continue; }
    size_t at = 0;
    int n = 0;
    size_t text_at = 0;
    uint64_t gun_spans = 0, gun_units = 0; /* --device-gunzip: spans and (bytes + spans) so far, from the files' sizes (a payload is shorter) */
    const int gz = elig[i] == 2; /* a batch holds files of one kind; its budget is counted in TEXT bytes either way */
    while (i + n < files->n && elig[i + n] == elig[i] && n < o->batch_files && (n == 0 || text_at + (gz ? gz_isize[i + n] : fsize[i + n]) <= o->batch_bytes)) {
      if (gz && o->gz_gunzip) {
        const uint64_t ns = (fsize[i + n] + gun_S - 1) / gun_S;
        if (n && (gun_spans + ns > MK_GUNZIP_BATCH_SPANS_MAX || (gun_units + fsize[i + n] + ns) * gun_R > MK_GUNZIP_BATCH_SYMS_MAX)) break;
        gun_spans += ns;
        gun_units += fsize[i + n] + ns;
      }
      foff[i + n] = at;
      if (gz) at += ((size_t)fsize[i + n] + 1023u) & ~(size_t)1023u; /* the file's bytes as they are */
      else if (batch_rows) { /* its place: the rows its text can give at most */
        /* (wide rows: an extension row for one row in sixteen -- a genome has them at contig ends and runs of N; a file with
         * more gets memory of its own, breader_run) */
        const uint64_t full = mk_fasta_pack_bound((size_t)fsize[i + n], P->TL, rows_format);
        slot_rows[i + n] = rows_format == MK_ROWS_WIDE ? full / 2u + full / 32u + 8u : full;
        at += (size_t)slot_rows[i + n] * MK_PACKED_PITCH;
      } else at += ((size_t)fsize[i + n] + 1023u) & ~(size_t)1023u;
      text_at += ((size_t)(gz ? gz_isize[i + n] : fsize[i + n]) + 1023u) & ~(size_t)1023u;
      n++;
    }
    if (at > bufcap) bufcap = at;
    jobs[njobs].first = i; jobs[njobs].n = n; jobs[njobs].batch = nbatches++; jobs[njobs].gz = gz; br->left[njobs] = n; njobs++;
    i += n;
  }
  b->nbatches = nbatches;
  br->files = &s->files; br->fsize = fsize; br->kind = elig; br->njobs = njobs;
  br->rows_TL = batch_rows ? P->TL : 0; br->rows_format = rows_format;
  br->bufcap = (bufcap + 4096 + (((size_t)2 << 20) - 1)) & ~(((size_t)2 << 20) - 1); /* whole 2 MiB granules: every buffer is pinned on its own */
}
/* the oldest batch in flight comes home: its files' sketches into the directory, its buffer back to the readers */
static void batch_end_oldest(batch_run *b) {
  stage1 *s = b->s;
  breader *br = &b->br;
  ctx_t *c = &s->c;
  const bjob *bj = &br->jobs[b->fly[0]];
  uint32_t *gzst = b->gzst;
  const double tf = now_s();
  const int rc = bj->nsub ? mk_sketch_batch_end(c->eng, b->bres) : MK_OK; /* (nsub == 0: every file of a gzip batch changed on disk) */
  s->t_finish += now_s() - tf;
  if (b->btrace) fprintf(stderr, "[batch %d] end: called %.3f returned %.3f ms\n", bj->batch, (tf - g_t0) * 1e3, (now_s() - g_t0) * 1e3);
  if (rc != MK_OK) die("mk_sketch_batch_end failed (%d): %s", rc, mk_last_error(c->eng));
  if (bj->gz && bj->nsub) (void)mk_sketch_batch_gz_status(c->eng, gzst, (uint32_t)bj->nsub);
  if (bj->gz && bj->nsub && g_opt.gz_gunzip) (void)mk_sketch_batch_gz_pieces(c->eng, b->gzpc, (uint32_t)bj->nsub);
  for (int k = 0; k < bj->n; k++) {
    const int i = bj->first + k;
    const char *path = s->files.v[i];
    const int p = bj->gz ? b->gzpos[i] : k; /* its result in bres */
    /* a gzip file the device route gave up with a status (more members behind the first, damage): again through zcat, which alone
     * decides whether the file is damaged -- with the messages and the exit status it has always had */
    const int gzfall = bj->gz && p >= 0 && gzst[p] != 0;
    if (gzfall) { br->grew[i] = 1; g_gz_fallback = g_opt.gz_gunzip ? mk_gunzip_status_text((int)gzst[p]) : mk_inflate_status_text((int)gzst[p]); }
    if (br->priv[i]) { free(br->priv[i]); br->priv[i] = NULL; }
    if (br->grew[i]) { /* longer than its place: alone, from the whole file, where it stands in the order */
      sketch_and_emit(s, i);
      g_gz_fallback = NULL;
      continue;
    }
    if (bj->gz && g_opt.gz_gunzip) {
      if (g_opt.timing) printf("{\"input\": \"%s\", \"route\": \"device-gunzip\", \"pieces\": %u, \"comp_bytes\": %llu, \"text_bytes\": %llu}\n", path, b->gzpc[p],
                               (unsigned long long)s->fsize[i], (unsigned long long)s->gz_isize[i]);
    } else if (bj->gz) {
      mk_bgzf_stats gs;
      memset(&gs, 0, sizeof gs);
      gs.blocks = 1; gs.chunks = 1; gs.comp_bytes = s->fsize[i]; gs.text_bytes = s->gz_isize[i];
      report_route(path, "device-inflate", &gs);
    }
    if (b->bres[p].status == MK_ERR_CROWDED) die("the context space is too crowd, try rerun the program using -k%d", s->P.k + 1);
    if (b->bres[p].status == MK_ERR_FORMAT) die("fasta2co(): can not find seqences head start from '>' 0 (%s ends inside a header line)", path);
    if (b->bres[p].status != MK_OK) die("sketching %s failed (%d)", path, b->bres[p].status);
    emit_result(s, i, NULL, &b->bres[p].r);
  }
  repoison(br->buf[bj->batch % br->nbufs], br->bufcap); /* (MK_POISON: the next batch in this buffer starts from the pattern) */
  pthread_mutex_lock(&br->mu); br->released++; pthread_cond_broadcast(&br->cv_free); pthread_mutex_unlock(&br->mu);
  b->fly[0] = b->fly[1]; b->nfly--;
}
/* a batch's buffer is pinned the first time it is used (the runtime is up by then) */
static void batch_pin(batch_run *b, int buf) {
  if (b->buf_pinned[buf]) return;
  const double tp = now_s();
  if (mk_host_register(b->br.buf[buf], b->br.bufcap) != MK_OK) die("pinning the batch buffers failed: %s", mk_last_error(NULL));
  b->buf_pinned[buf] = 1;
  b->s->t_batch_pin += now_s() - tp;
}
static void run_batches(stage1 *s, batch_run *b) {
  const cli_opts *o = &g_opt;
  breader *br = &b->br;
  ctx_t *c = &s->c;
  bjob *jobs = br->jobs;
  const int batch_rows = b->batch_rows, nbatches = b->nbatches;
  pthread_mutex_init(&br->mu, NULL); pthread_cond_init(&br->cv_ready, NULL); pthread_cond_init(&br->cv_free, NULL);
  /* the buffers: mapped and touched now, so that the readers can start while the runtime and the engine come up; pinned when the
   * first batch is handed over (see cli_sink_alloc) */
  /* Rows: the readers may run AHEAD by as many batches as 2 GiB of buffers hold -- the 75 ms the runtime and the engine's queue
   * take to come up are time to walk and pack in (1 024 genomes of 4 Mbases are 2 GB of rows: all of them are packed by then, and
   * what is left is the link's time); the pages are touched by the readers as they write.  Text: four buffers, touched here. */
  int want_bufs = BATCH_BUFS;
  if (batch_rows) {
    want_bufs = (int)((((size_t)2 << 30) + br->bufcap - 1) / br->bufcap);
    if (want_bufs < BATCH_BUFS) want_bufs = BATCH_BUFS;
    if (want_bufs > BATCH_BUFS_MAX) want_bufs = BATCH_BUFS_MAX;
  }
  const int nbufs = br->nbufs = nbatches < want_bufs ? nbatches : want_bufs;
  size_t arena_len = 0;
  uint8_t *arena = batch_rows ? arena_map_untouched((size_t)nbufs * br->bufcap, &arena_len) : arena_map_unpinned((size_t)nbufs * br->bufcap, &arena_len);
  if (!arena) die("out of memory (%zu bytes of batch buffers)", (size_t)nbufs * br->bufcap);
  repoison(arena, arena_len); /* (MK_POISON: fresh anonymous pages are zeros otherwise) */
  for (int k = 0; k < nbufs; k++) br->buf[k] = arena + (size_t)k * br->bufcap;
  /* (rows: 16 readers by default.  On the 64-core host 1 024 genomes of 4 Mbases took 0.108-0.113 s with 16, 0.114-0.118 with 24,
   * 0.120-0.132 with 32 and up to 0.23 with 48: 16 pack the directory inside the runtime's start-up (5-6 GB/s of text each), and every
   * further thread is memory traffic beside that start-up -- the engine is ready at 0.078-0.084 s with 16 readers, 0.088-0.093 with
   * 24, 0.095-0.107 with 32) */
  int nreaders = s->nthreads < 1 ? 1 : (s->nthreads > 64 ? 64 : s->nthreads);
  if (batch_rows && !o->threads_given && nreaders > 16) nreaders = 16;
  pthread_t readers[64];
  int started = 0;
  for (int t = 0; t < nreaders; t++) if (pthread_create(&readers[started], NULL, breader_run, br) == 0) started++;
  if (!started) die("cannot start a thread: %s", strerror(errno));
  c->nthreads = s->nthreads;
  s->jo.nworkers = 0;
  const int mode = o->uniq ? MK_MODE_UNIQ_SET : MK_MODE_SET;
  mk_batch_file *bf = b->bf = calloc((size_t)o->batch_files, sizeof *bf);
  b->bres = calloc((size_t)o->batch_files, sizeof *b->bres);
  mk_gz_file *gzf = b->gzf = calloc((size_t)o->batch_files, sizeof *gzf);
  b->gzst = calloc((size_t)o->batch_files, sizeof *b->gzst); b->gzpc = calloc((size_t)o->batch_files, sizeof *b->gzpc);
  if (!bf || !b->bres || !gzf || !b->gzst || !b->gzpc) die("out of memory");
  b->btrace = getenv("MK_BATCH_TRACE") != NULL;
  for (int j = 0; j < br->njobs; j++) {
    const bjob *bj = &jobs[j];
    if (bj->batch < 0) { /* one file alone, in its place: everything in front of it comes home first */
      while (b->nfly) batch_end_oldest(b);
      sketch_and_emit(s, bj->first);
      continue;
    }
    {
      const double tw = now_s();
      pthread_mutex_lock(&br->mu);
      while (br->left[j] > 0) pthread_cond_wait(&br->cv_ready, &br->mu);
      pthread_mutex_unlock(&br->mu);
      s->t_batch_wait_read += now_s() - tw;
    }
    int nsub = bj->n;
    if (bj->gz) nsub = 0;
    for (int k = 0; k < bj->n && bj->gz; k++) { /* the bytes the readers got, looked at again: a file that changed since it was planned is sketched alone */
      const int i = bj->first + k;
      b->gzpos[i] = -1;
      if (br->failed[i]) die("%s: %s", s->files.v[i], strerror(br->failed[i]));
      if (br->grew[i]) continue;
      mk_gzip_info gi;
      uint8_t *at = br->buf[bj->batch % nbufs] + br->foff[i];
      if (mk_gzip_scan(-1, at, (size_t)s->fsize[i], &gi) != MK_OK || !gi.is_single || gi.isize != s->gz_isize[i]) { br->grew[i] = 1; continue; }
      gzf[nsub].comp = at; gzf[nsub].n = s->fsize[i]; gzf[nsub].info = gi;
      b->gzpos[i] = nsub++;
    }
    jobs[j].nsub = nsub;
    for (int k = 0; k < bj->n && !bj->gz; k++) {
      const int i = bj->first + k;
      if (br->failed[i] == -MK_ERR_FORMAT + 100000) die("fasta2co(): can not find seqences head start from '>' 0 (%s ends inside a header line)", s->files.v[i]);
      if (br->failed[i]) die("%s: %s", s->files.v[i], strerror(br->failed[i]));
      bf[k].text = br->priv[i] ? br->priv[i] : br->buf[bj->batch % nbufs] + br->foff[i];
      bf[k].n = batch_rows ? br->nrows[i] * MK_PACKED_PITCH : s->fsize[i];
    }
    (void)engine_get(c);
    /* the runtime is up now.  Buffer by buffer: only the first buffer's pinning lies in front of the first batch, every other buffer
     * is pinned behind the begin of the batch in front of it (below), while the device works */
    batch_pin(b, bj->batch % nbufs);
    if (b->nfly == 2) batch_end_oldest(b);
    if (c->t_first_push == 0) c->t_first_push = now_s() - g_t0;
    int rc;
    {
      const double tb = now_s();
      if (bj->gz && o->gz_gunzip) {
        const mk_gunzip_opts go = {o->gunzip_opts.span_bytes, o->gunzip_opts.ratio, 0u, 0u}; /* (members are out of scope in batches: such a file falls back) */
        rc = nsub ? mk_sketch_batch_begin_gunzip(c->eng, mode, gzf, (uint32_t)nsub, &go) : MK_OK;
      } else if (bj->gz) rc = nsub ? mk_sketch_batch_begin_gz(c->eng, mode, gzf, (uint32_t)nsub) : MK_OK;
      else rc = batch_rows ? mk_sketch_batch_begin_rows(c->eng, mode, br->rows_format, bf, (uint32_t)bj->n) : mk_sketch_batch_begin(c->eng, mode, bf, (uint32_t)bj->n);
      s->t_batch_begin += now_s() - tb;
      s->nbatches_done++;
      if (b->btrace) fprintf(stderr, "[batch %d] begin: called %.3f returned %.3f ms\n", bj->batch, (tb - g_t0) * 1e3, (now_s() - g_t0) * 1e3);
    }
    if (rc != MK_OK) die("mk_sketch_batch_begin failed (%d): %s", rc, mk_last_error(c->eng));
    c->t_last_push = now_s() - g_t0;
    b->fly[b->nfly++] = j;
    if (bj->batch + 1 < nbatches) batch_pin(b, (bj->batch + 1) % nbufs); /* the next batch's buffer, beside this batch's kernels */
  }
  while (b->nfly) batch_end_oldest(b);
  for (int t = 0; t < started; t++) pthread_join(readers[t], NULL);
  s->t_readers_read = br->cpu_read; s->t_readers_pack = br->cpu_pack; s->t_readers_blocked = br->cpu_blocked;
  (void)engine_get(c);
}
/* several engines, whole files each */
static void run_sharded(stage1 *s) {
  const cli_opts *o = &g_opt;
  ctx_t *c = &s->c;
  const int ndev = o->ndev;
  shard_driver *drv = calloc((size_t)ndev, sizeof *drv);
  file_result *results = calloc((size_t)s->files.n, sizeof *results);
  pthread_mutex_t smu = PTHREAD_MUTEX_INITIALIZER;
  pthread_cond_t scv = PTHREAD_COND_INITIALIZER;
  int cursor = 0;
  if (!drv || !results) die("out of memory");
  c->nthreads = s->nthreads;
  (void)engine_get(c); /* engine 0 (devs[0]) from the start-up thread */
  for (int j = 0; j < ndev; j++) {
    shard_driver *d = &drv[j];
    d->o = &s->jo; d->device = o->devs[j]; d->cursor = &cursor; d->out = results; d->mu = &smu; d->cv = &scv;
    d->c.chunk_bytes = o->chunk_bytes; d->c.drop_pages = o->drop_pages; d->c.inflight = o->inflight; d->c.direct_host = o->direct_host;
    d->c.ndev = 1;
    if (j == 0) { d->c.eng = c->eng; d->c.engs[0] = c->eng; }
    if (pthread_create(&d->th, NULL, shard_driver_run, d) != 0) die("cannot start a thread: %s", strerror(errno));
  }
  for (int i = 0; i < s->files.n; i++) {
    pthread_mutex_lock(&smu);
    while (!results[i].ready) pthread_cond_wait(&scv, &smu);
    file_result fr = results[i];
    pthread_mutex_unlock(&smu);
    emit_result(s, i, NULL, &fr.res);
    free_result(&fr.res);
  }
  for (int j = 0; j < ndev; j++) { pthread_join(drv[j].th, NULL); s->t_finish += drv[j].t_finish; c->nrows_total += drv[j].c.nrows_total; }
}
/* many files on one GPU: up to four engines take the files in turn and ONE thread drives them all -- a file is begun and
 * pushed on an engine that is free (copy and kernels queued on its stream); when none is free the oldest file in flight is
 * finished on its engine: while the host waits there and writes the result, the GPU already works on the files behind it,
 * and the small kernels of neighbouring files overlap.  (With a single engine the GPU idles through every host round trip:
 * 160 us of kernels and 75 us of copy per 4 Mbase genome against 420 us per genome in steady state.)  Engines join as they
 * come up (21 GB of tables at L2K11 take anything from 0.04 to 1 s each beside a working GPU): until then fewer take turns. */
static void run_engines(stage1 *s) {
  const cli_opts *o = &g_opt;
  extra_engines_t *extra = &s->extra;
  const int nfiles = s->files.n, n_engines = s->n_engines;
  ctx_t cx[MAX_ENGINES_PER_GPU];
  cx[0] = s->c;
  (void)engine_get(&cx[0]);
  int have = 1; /* engines in use */
  struct { int file, eng, held; } fly[MAX_ENGINES_PER_GPU]; /* files in flight, oldest first */
  int nfly = 0, busy[MAX_ENGINES_PER_GPU] = {0, 0, 0, 0}, extra_warned = 0;
  for (int i = 0; i < nfiles || nfly; ) {
    if (__atomic_load_n(&extra->failed, __ATOMIC_ACQUIRE) && !extra_warned) {
      /* the extra engines are a speed-up that is on by default: one that does not come up (a smaller or shared GPU: an L2K11
       * engine is 21 GB of tables) must not turn a run that works on one engine into an error -- unless --engines asked for them */
      if (o->engines_per_gpu) die("mk_engine_create (engine %d of %d, --engines %d) failed: %s", have + 1, n_engines, o->engines_per_gpu, extra->err);
      fprintf(stderr, "metakssd: warning: engine %d of %d did not come up (%s): going on with %d\n", 1 + __atomic_load_n(&extra->ready, __ATOMIC_ACQUIRE) + 1,
              n_engines, extra->err, 1 + __atomic_load_n(&extra->ready, __ATOMIC_ACQUIRE));
      extra_warned = 1;
    }
    const int ready = 1 + __atomic_load_n(&extra->ready, __ATOMIC_ACQUIRE);
    while (have < ready) { /* a new engine: its own buffers for files that stream */
      cx[have] = cx[0];
      cx[have].io = NULL; cx[have].rows = NULL; cx[have].arena = NULL; cx[have].arena_bytes = 0; cx[have].nrows_total = 0;
      cx[have].pin = NULL; /* (the first engine's pinner stays the first engine's: cli_sink_alloc destroys the one it finds beside a new arena) */
      cx[have].eng = extra->eng[have - 1]; cx[have].engs[0] = extra->eng[have - 1]; cx[have].ndev = 1; cx[have].multi = NULL;
      engine_apply_options(&cx[have], cx[have].eng);
      have++;
    }
    int e = -1;
    if (i < nfiles)
      for (int k = 0; k < have; k++) if (!busy[k]) { e = k; break; }
    if (e >= 0) {
      fly[nfly].file = i; fly[nfly].eng = e; fly[nfly].held = -1;
      sketch_file_push(&cx[e], &s->jo, i, &fly[nfly].held);
      busy[e] = 1; nfly++; i++;
      continue;
    }
    /* every engine has a file (or the files are out): the oldest comes home */
    const int j = fly[0].file, ej = fly[0].eng;
    mk_result res;
    sketch_file_finish(&cx[ej], &s->jo, j, fly[0].held, &res, &s->t_finish);
    emit_result(s, j, cx[ej].eng, &res);
    busy[ej] = 0;
    for (int k = 1; k < nfly; k++) fly[k - 1] = fly[k];
    nfly--;
  }
  /* engines that come up after the last file are not used; the fast exit below does not wait for them */
  if (o->slow_exit || s->stage2_after) pthread_join(extra->th, NULL);
  uint64_t rows_all = 0;
  for (int k = 0; k < have; k++) rows_all += cx[k].nrows_total;
  s->c.nrows_total = rows_all;
  s->c.eng = cx[0].eng;
}
static void run_serial(stage1 *s) {
  for (int i = 0; i < s->files.n; i++) sketch_and_emit(s, i);
}
/* worker threads prepare files ahead when there are several inputs */
static void start_prefetch(stage1 *s, int first_nonfq) {
  const cli_opts *o = &g_opt;
  pf_t *pf = &s->pf;
  const int nfiles = s->files.n;
  pthread_t workers[PF_MAX_BUFS];
  int nworkers = 0;
  pf->files = &s->files; pf->TL = s->P.TL;
  pf->qmin = o->kmerqlty;
  pf->koc_until = o->abundance ? first_nonfq : 0; /* files in front of this index are read the mt_shortreads2koc way */
  pf->nbufs = s->nthreads < PF_MAX_BUFS ? s->nthreads : PF_MAX_BUFS;
  if (s->shard_files && pf->nbufs < o->ndev + 1) pf->nbufs = o->ndev + 1 < PF_MAX_BUFS ? o->ndev + 1 : PF_MAX_BUFS; /* every driver may hold one */
  if (pf->nbufs < s->n_engines + 1) pf->nbufs = s->n_engines + 1; /* every engine in turn holds one while its file is in flight (4 + 1 <= PF_MAX_BUFS) */
  if (pf->nbufs > nfiles) pf->nbufs = nfiles;
  pf->slots = calloc(nfiles, sizeof(pf_slot));
  pthread_mutex_init(&pf->mu, NULL); pthread_cond_init(&pf->cv_buf, NULL); pthread_cond_init(&pf->cv_ready, NULL);
  /* one pinned block for all row buffers (an anonymous mapping touched in parallel and registered once): sixteen
   * hipHostMalloc calls of 64 MiB took 0.2 s of a 0.9 s run over 1024 genomes */
  void *arena = NULL;
  if (mk_host_arena_alloc(&arena, (size_t)pf->nbufs * ROWBUF) == MK_OK) {
    for (int k = 0; k < pf->nbufs; k++) {
      pf->bufs[k] = (uint8_t *)arena + (size_t)k * ROWBUF;
      pf->free_bufs[pf->nfree++] = k;
    }
  } else {
    for (int k = 0; k < pf->nbufs; k++) {
      if (mk_host_alloc((void **)&pf->bufs[k], ROWBUF) != MK_OK) { pf->nbufs = k; break; }
      pf->free_bufs[pf->nfree++] = k;
    }
  }
  for (int t = 0; t < pf->nbufs; t++)
    if (pthread_create(&workers[nworkers], NULL, pf_worker, pf) == 0) nworkers++;
  if (nworkers == 0) { free(pf->slots); pf->slots = NULL; }
  s->jo.nworkers = nworkers;
}
/* --timing: one JSON line for bench.py / tools: seconds since process start unless named *_s */
static void print_timing(const stage1 *s) {
  const ctx_t *c = &s->c;
  printf("{\"timing\": {\"t0_abs\": %.6f, \"exit_abs\": %.6f, \"shuf_read\": %.4f, \"hip_ready\": %.4f, \"engine_ready\": %.4f, \"first_push\": %.4f, \"last_push\": %.4f, \"unmapped\": %.4f, "
         "\"written\": %.4f, \"finish_s\": %.4f, \"begin_s\": %.4f, \"rows\": %llu, \"threads\": %u, \"chunks\": %llu, \"chunks_discarded\": %llu, "
         "\"serial_rows\": %llu, \"stream_setup_s\": %.4f, \"stream_wait_frame_s\": %.4f, \"stream_push_s\": %.4f, \"stream_total_s\": %.4f, "
         "\"push_call_s\": %.4f, \"wait_call_s\": %.4f, \"push_call_max_s\": %.4f, \"first_push_call_s\": %.4f, \"gpus\": %d, \"gather_ms\": %.3f, \"tail_ms\": %.3f, \"transport\": \"%s\", "
         "\"batches\": %d, \"batch_wait_readers_s\": %.4f, \"batch_pin_s\": %.4f, \"batch_begin_s\": %.4f, "
         "\"readers_read_cpu_s\": %.4f, \"readers_pack_cpu_s\": %.4f, \"readers_blocked_s\": %.4f, "
         "\"pin_calls\": %d, \"pin_s\": %.4f, \"pinned_mib\": %.1f, \"pool_mib\": %.1f}}\n",
         g_t0, now_s(), s->t_shuf, s->fut.t_hip_ready, s->fut.t_ready, c->t_first_push, c->t_last_push, c->t_unmapped, s->t_written, s->t_finish, c->t_begin_s, (unsigned long long)c->nrows_total,
         c->fq_stats.threads, (unsigned long long)c->fq_stats.chunks, (unsigned long long)c->fq_stats.chunks_discarded,
         (unsigned long long)c->fq_stats.serial_rows, c->fq_stats.t_setup_s, c->fq_stats.t_wait_frame_s, c->fq_stats.t_push_s,
         c->fq_stats.t_total_s, c->fq_stats.t_push_call_s, c->fq_stats.t_wait_call_s, c->fq_stats.t_push_call_max_s,
         c->fq_stats.t_first_push_call_s, c->ndev ? c->ndev : 1, c->gather_ms, c->tail_ms, c->multi ? g_multi.transport(c->multi) : "-",
         s->nbatches_done, s->t_batch_wait_read, s->t_batch_pin, s->t_batch_begin, s->t_readers_read, s->t_readers_pack, s->t_readers_blocked,
         c->pin ? c->pin->calls : 0, c->pin ? c->pin->t_pin_s : 0.0, c->pin ? (double)c->pin->pinned_bytes / 1048576.0 : 0.0, (double)c->arena_bytes / 1048576.0);
}
int run_stage1(int stage2_after) {
  cli_opts *o = &g_opt; /* (the genome routes of --device-gunzip are settled here) */
  static stage1 S;      /* (zeroed; it holds the start-up future and the contexts the worker threads point into) */
  static batch_run B;
  stage1 *s = &S;
  strlist *files = &s->files;
  const int ndev = o->ndev, device = o->device;
  s->quiet = o->quiet; s->stage2_after = stage2_after; s->nthreads = o->nthreads;
  discover(files, o->args.n, o->args.v);
  if (files->n == 0) die("not valid raw seq format");
  fused_t *fu = &s->fu;
  if (o->composite_db) { /* (the other refusals of the fused route: dist_dispatch(); all of them before the device is touched) */
    for (int i = 0; i < files->n; i++)
      if (!is_fastq(files->v[i])) die("--composite takes FASTQ inputs: %s is none", files->v[i]);
    fu->on = 1; fu->refdir = o->composite_db; fu->abv_dir = o->abv_dir ? o->abv_dir : "./"; fu->device = device;
    fu->batch_limit = o->batch_given ? (uint64_t)o->batch_bytes : 256ull << 20; /* composite's --batch-mib */
    o->batch_bytes = 0;
    fu->rhave = costat_load(fu->refdir, &fu->rs);
    if (fu->rhave == COSTAT_ABSENT) die("cannot find cofiles.stat under %s ", fu->refdir);
  }

  const double t0 = g_t0;
  /* HIP start-up and then the engine's tables on a helper thread; the main thread reads the .shuf file meanwhile and goes
   * on to map and frame the input */
  /* several GPUs and several files: the files are dealt to the GPUs whole (no exchange, no RCCL); several GPUs and ONE file: its
   * rows are dealt round-robin and the partial sketches merged on GPU 0 (libmetakssd_multi.so) */
  const int shard_files = s->shard_files = ndev > 1 && files->n > 1;
  engine_start(&s->fut, ndev ? o->devs[0] : device, o->devs, shard_files ? 0 : ndev, o->allow_copies ? MK_MULTI_ALLOW_DEVICE_COPIES : 0u);
  mk_params *P = &s->P;
  /* the marker database goes up beside the engine's start-up and the first file's reading; fused_sample() waits for it */
  if (fu->on && pthread_create(&fu->th, NULL, fused_load_run, fu) != 0) die("cannot start a thread: %s", strerror(errno));
  load_shuf_params(o->shuf_path, &s->sh, P);
  if (fu->on) { /* cmd_composite()'s checks of the two headers, in its order */
    if ((uint32_t)P->shuf_id != fu->rs.shuf_id) printf("get_species_abundance(): qry shuf_id %u not match ref shuf_id: %u\n", (uint32_t)P->shuf_id, fu->rs.shuf_id);
    if (fu->rhave < COSTAT_FULL) die("get_species_abundance(): truncated cofiles.stat");
    if (fu->rs.comp_num != P->component_num || P->component_num > 16)
      die("--composite: the marker database has %d components, the sketch %d (equal and at most 16)", fu->rs.comp_num, P->component_num);
    fu->vec = malloc(8 * ((size_t)fu->rs.infile_num + 1));
    fu->row_end = malloc(8 * ((size_t)files->n + 1));
    if (!fu->vec || !fu->row_end) die("out of memory");
    s->c.want_keys = 1;
  }
  if (!s->quiet) printf("rand_id=%d\thalf_ctx_len=%d\thashsize=%u\thashlimit=%u\n", P->shuf_id, P->k, P->hashsize, P->hashlimit);
  s->t_shuf = now_s() - t0;

  /* --device-gunzip also plans single-member .gz genomes into gz batches, as --device-inflate does; --no-device-inflate turns both off */
  if (o->device_gunzip && !o->no_device_inflate) { o->gz_batches = 1; o->gz_gunzip = 1; }
  /* S and R of that route as the library will clamp them: a batch is planned inside its two limits (mk_sketch_batch_begin_gunzip) */
  s->gun_S = o->gunzip_opts.span_bytes ? (o->gunzip_opts.span_bytes < 64u ? 64u : o->gunzip_opts.span_bytes > (1u << 30) ? (1u << 30) : o->gunzip_opts.span_bytes)
                                       : MK_GUNZIP_BATCH_SPAN_DEFAULT;
  s->gun_R = o->gunzip_opts.ratio ? (o->gunzip_opts.ratio > 65536u ? 65536u : o->gunzip_opts.ratio) : 16u;
  { /* a directory of genomes goes to the device in batches of files, each file with a small table of its own: the engine's
     * hashsize-slot tables (21 GB at L2K11) are then made only if a file falls out of its batch (MK_ENGINE_LAZY_TABLES) */
    int plain = 0;
    for (int i = 0; i < files->n; i++) plain += !is_fastq(files->v[i]) && (!is_compressed(files->v[i]) || (o->gz_batches && has_suffix(files->v[i], ".gz")));
    s->fut.lazy_tables = plain >= 2 && !o->no_batch && !o->host_fasta && !o->engines_per_gpu && !shard_files && ndev <= 1;
  }
  engine_params(&s->fut, P);
  /* more engines on the same GPU for directories of many files (see the file loop), created beside the first and joining as
   * they come up.  Two by default, four at most: 1024 genomes of 4 Mbases at L3K10 go through at 3 750 genomes/s with one engine,
   * 6 100-6 400 with two, 5 650-6 150 with three, 5 570-5 860 with four (from "engine ready" to "directory written", one box,
   * tools/gpu_session_r3x.sh); at L2K11 (21 GB of tables per engine) at 2 600 / 4 450 / 2 100-4 700 / 1 700-2 000 -- creating 21 GB
   * engines beside a working one takes 0.04 to 1 s each, two pay, more do not.  --engines 1 turns it off */
  if (o->engines_per_gpu < 0 || o->engines_per_gpu > MAX_ENGINES_PER_GPU) die("--engines takes 1..%d", MAX_ENGINES_PER_GPU);
  plan_batches(s, &B);
  const int n_engines = s->n_engines = (!s->use_batch && !shard_files && ndev <= 1 && files->n >= 8 && !fu->on && !o->long_reads && !o->long_reads_q) ? (o->engines_per_gpu ? o->engines_per_gpu : MK_DEFAULT_ENGINES) : 1;
  if (n_engines > 1) {
    s->extra.P = P; s->extra.device = ndev ? o->devs[0] : device; s->extra.want = n_engines - 1;
    if (pthread_create(&s->extra.th, NULL, extra_engines_run, &s->extra) != 0) die("cannot start a thread: %s", strerror(errno));
  }
  ctx_t *c = &s->c;
  c->fut = &s->fut;
  c->chunk_bytes = o->chunk_bytes; c->drop_pages = o->drop_pages; c->inflight = o->inflight; c->direct_host = o->direct_host;
  c->packed = !o->ascii_rows && mk_params_packed_ok(P);
  c->bgzf_ok = ndev <= 1 && n_engines == 1 && !shard_files;
  /* packed rows are 64 bytes a read on PCIe instead of 160: the framers, not the link, bound a FASTQ file then, and 32 of them did
   * better than 24 (50 M reads: 0.20-0.24 s against 0.22-0.26 from process start; 48 and more are slower again) */
  if (c->packed && !o->threads_given && o->ncpu >= 32) s->nthreads = 32;

  /* -A stays on only if every input is FASTQ: the reference switches it off when its file loop reaches the first
   * non-FASTQ input (command_dist.c:389-392) and then writes no combco.N.a at all (:427-431).  FASTQ files in front of
   * that point have by then been sketched by mt_shortreads2koc() + write_fqkoc2files() (every key, -n / -Q ignored), the
   * ones behind it go through fastq2co(): the same here, in our file order. */
  int first_nonfq = files->n;
  for (int i = files->n - 1; i >= 0; i--)
    if (!is_fastq(files->v[i])) first_nonfq = i;
  const int koc_dir = o->abundance && first_nonfq == files->n;
  int rc = fu->on ? MK_OK : mk_sketchdir_open(o->outdir, P, koc_dir, files->n, &s->sd);
  if (rc != MK_OK) die("cannot create sketch directory %s (%d)", o->outdir, rc);
  s->jo = (job_opts){files, P, o->abundance, o->uniq, first_nonfq, o->kmerocrs, o->kmerqlty, s->nthreads, s->quiet, &s->pf, 0};
  if (files->n > 1 && s->nthreads > 1 && !s->use_batch && !o->long_reads && !o->long_reads_q) start_prefetch(s, first_nonfq); /* (its workers frame FASTQ files into rows) */
  if (first_nonfq < files->n && o->abundance) printf("Warning: close abundance mode (-A) since non-fastq file input.\n");
  if (s->use_batch) run_batches(s, &B);
  else if (shard_files) run_sharded(s);
  else if (n_engines > 1) run_engines(s);
  else run_serial(s);
  if (!s->quiet) printf("\n");
  rc = fu->on ? MK_OK : mk_sketchdir_close(s->sd);
  if (rc != MK_OK) die("closing sketch directory failed (%d)", rc);
  s->t_written = now_s() - t0;
  if (!s->quiet) printf("sketched %llu rows from %d file(s) in %.3f s\n", (unsigned long long)c->nrows_total, files->n, s->t_written);
  if (o->timing) print_timing(s);
  if (o->timing && fu->on)
    printf("{\"composite_timing\": {\"route\": \"device\", \"samples\": %d, \"batches\": %llu, \"hits\": %llu, \"load_kernel_ms\": %.3f, \"query_kernel_ms\": %.3f}}\n",
           files->n, (unsigned long long)fu->batches, (unsigned long long)fu->hits, fu->load_ms, fu->query_ms);
  if (stage2_after) {
    if (c->rows) mk_host_free(c->rows);
    free(c->io);
    if (!c->multi) mk_engine_destroy(engine_get(c));
    mk_shuf_free(&s->sh);
    return run_stage2(o->outdir, o->outdir, device, s->quiet);
  }
  if (o->slow_exit) { /* profilers collect their data in exit handlers */
    if (!c->multi) mk_engine_destroy(engine_get(c));
    return 0;
  }
  /* everything is on disk: leave without tearing down 2 GB of device tables and the pinned pools page by page */
  fflush(stdout);
  fflush(stderr);
  _exit(0);
}
