/*
 * host_pipe.c - everything that takes HOST pointers, plain C.
 *
 * The reference's functions take ordinary (malloc) memory, are reentrant and scale with the caller's threads
 * (reference lib/eddsa.h:44-80).  Three pieces give the GPU engine the same manners:
 *
 *   1. A streaming pipeline over PIPE_LANES lanes.  A lane carries one chunk of the batch at a time on its own
 *      stream - upload, kernels, download, in order - so up to three chunks are in flight: one uploading, one
 *      computing, one downloading, and the kernels of consecutive chunks overlap on the GPU (each lane's stream
 *      draws its own workspace from the engine's pool).  Chunks start small (2^16 or 2^17 items: the GPU is working
 *      0.2 ms after the call) and double up to the job's stage size.
 *   2. Pinned staging.  hipMemcpyAsync from pageable memory is staged by the HIP runtime on one thread at about
 *      11 GB/s and blocks the caller (round 2: 86.8 M verifies/s host to host against 109.5 kernel-only, sign 113
 *      against 182 from pinned memory).  Here every lane owns pinned staging buffers; caller memory is copied into
 *      them by a small pool of copier threads, piece by piece, each piece handed to the DMA engine as soon as it is
 *      staged; results come back the same way.  Caller memory that is already pinned (eddsa_amd_host_alloc,
 *      hipHostMalloc, hipHostRegister) is used in place.
 *   3. A combiner for concurrent small calls (flat combining).  A GPU pass costs about 0.4 ms however few items it
 *      carries, so T threads that each loop over ed25519_verify would get 1 / 0.4 ms verifies per second IN TOTAL
 *      if their calls ran one after the other.  Instead a small call queues its request; one of the waiting
 *      threads becomes the leader of its operation, packs everything queued for that operation into one batch, runs
 *      it as a single pipeline job (one lane: the launches of different operations overlap) and hands the results back.
 *
 * Jobs that carry secrets (secret keys, scalars, shared secrets) zero their staging copies - in HBM, in the
 * pinned host buffers and in the combiner's buffers - before the call returns, on the error path too (the
 * reference wipes its stack after the same operations: lib/ed25519-sha512.c:77,136, lib/x25519.c:208,221).
 *
 * What an operation is - widths, wipes, chunk sizes, combiner slot - is one row of the table g_ops; a call (struct hjob) is
 * a row and its pointers.  The measurement aids and test hooks of the debug library stand together at the end of the file.
 */
#define _GNU_SOURCE                    /* syscall(): the combiner's waiters sleep on a futex */
#include "engine.h"

#include <limits.h>
#include <linux/futex.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/syscall.h>
#include <time.h>
#include <unistd.h>

/* ------------------------------------------------------------------------------------------
 * copier pool: memcpy / memset of large host ranges on several threads
 * ---------------------------------------------------------------------------------------- */

#define POOL_MAX_THREADS 16
#define POOL_QUEUE 256
#define POOL_MIN_SLICE ((size_t)1 << 20)     /* below 2 slices of this the caller copies by itself */

struct ptask { uint8_t *dst; const uint8_t *src; size_t bytes; int *pending; };   /* src == NULL: zero fill */

static struct {
    pthread_mutex_t lk;
    pthread_cond_t work_cv, done_cv;
    pthread_t th[POOL_MAX_THREADS];
    int started, want, stop;
    struct ptask q[POOL_QUEUE];
    unsigned head, tail;                      /* tasks q[head % POOL_QUEUE .. tail) */
} g_pool = { PTHREAD_MUTEX_INITIALIZER, PTHREAD_COND_INITIALIZER, PTHREAD_COND_INITIALIZER, {0}, 0, 6, 0, {{0}}, 0, 0 };

static void ptask_run(const struct ptask *t)
{
    if (t->src) memcpy(t->dst, t->src, t->bytes); else memset(t->dst, 0, t->bytes);
}

static void *pool_worker(void *arg)
{
    (void)arg;
    pthread_mutex_lock(&g_pool.lk);
    for (;;) {
        while (!g_pool.stop && g_pool.head == g_pool.tail) pthread_cond_wait(&g_pool.work_cv, &g_pool.lk);
        if (g_pool.head == g_pool.tail) break;   /* stopping, and nothing queued is left undone */
        struct ptask t = g_pool.q[g_pool.head++ % POOL_QUEUE];
        pthread_mutex_unlock(&g_pool.lk);
        ptask_run(&t);
        pthread_mutex_lock(&g_pool.lk);
        if (--*t.pending == 0) pthread_cond_broadcast(&g_pool.done_cv);
    }
    pthread_mutex_unlock(&g_pool.lk);
    return NULL;
}

/* helper threads beside the calling thread (default 6; 0 = the caller copies alone).  Takes effect for the threads
 * not yet started; eddsa_amd_shutdown stops the pool, the next large call starts it again. */
void eddsa_amd_set_host_threads(int n)
{
    pthread_mutex_lock(&g_pool.lk);
    g_pool.want = n < 0 ? 0 : n > POOL_MAX_THREADS ? POOL_MAX_THREADS : n;
    pthread_mutex_unlock(&g_pool.lk);
}

/* (two threads may shut the library down at once: the second waits for the first one's joins instead of joining the
 * same threads again) */
void host_pool_stop(void)
{
    pthread_mutex_lock(&g_pool.lk);
    while (g_pool.stop) pthread_cond_wait(&g_pool.done_cv, &g_pool.lk);
    const int n = g_pool.started;
    g_pool.stop = 1;
    pthread_cond_broadcast(&g_pool.work_cv);
    pthread_mutex_unlock(&g_pool.lk);
    for (int i = 0; i < n; i++) pthread_join(g_pool.th[i], NULL);
    pthread_mutex_lock(&g_pool.lk);
    g_pool.started = 0;
    g_pool.stop = 0;
    pthread_cond_broadcast(&g_pool.done_cv);
    pthread_mutex_unlock(&g_pool.lk);
}

/* Queue dst[0..bytes) = src[0..bytes) (src == NULL: zeros) for the pool, in slices; *pending counts the slices still
 * to be done (read and written under the pool's lock only; pool_wait).  What the pool cannot take - no helper threads,
 * no room in the queue - is done here and now.  Returns the bytes queued. */
static size_t pool_submit(int *pending, uint8_t *d, const uint8_t *s, size_t bytes, size_t slice)
{
    size_t off = 0;
    if (bytes >= POOL_MIN_SLICE) {
        pthread_mutex_lock(&g_pool.lk);
        while (g_pool.started < g_pool.want && !g_pool.stop) {
            if (pthread_create(&g_pool.th[g_pool.started], NULL, pool_worker, NULL) != 0) break;
            g_pool.started++;
        }
        if (g_pool.started > 0 && !g_pool.stop) {   /* (a pool that is being stopped takes no new work: done here instead) */
            if (slice == 0) {
                size_t parts = bytes / POOL_MIN_SLICE;
                if (parts > (size_t)g_pool.started) parts = (size_t)g_pool.started;
                slice = ((bytes + parts - 1) / parts + 4095) & ~(size_t)4095;
            }
            int added = 0;
            while (off < bytes && g_pool.tail - g_pool.head < POOL_QUEUE) {
                const size_t b = bytes - off < slice ? bytes - off : slice;
                const struct ptask t = { d + off, s ? s + off : NULL, b, pending };
                g_pool.q[g_pool.tail++ % POOL_QUEUE] = t;
                ++*pending;
                added++;
                off += b;
            }
            if (added) pthread_cond_broadcast(&g_pool.work_cv);
        }
        pthread_mutex_unlock(&g_pool.lk);
    }
    if (off < bytes) { const struct ptask t = { d + off, s ? s + off : NULL, bytes - off, NULL }; ptask_run(&t); }
    return off;
}

static void pool_wait(int *pending)
{
    pthread_mutex_lock(&g_pool.lk);
    while (*pending) pthread_cond_wait(&g_pool.done_cv, &g_pool.lk);
    pthread_mutex_unlock(&g_pool.lk);
}

/* dst[0..bytes) = src[0..bytes) (src == NULL: zeros) on the caller and the pool together; returns when all of it is done */
static void par_copy(void *dst, const void *src, size_t bytes)
{
    uint8_t *d = (uint8_t *)dst;
    const uint8_t *s = (const uint8_t *)src;
    int pending = 0;
    size_t own = bytes;
    if (bytes >= 2 * POOL_MIN_SLICE) {
        pthread_mutex_lock(&g_pool.lk);
        const size_t helpers = (size_t)(g_pool.started > g_pool.want ? g_pool.started : g_pool.want);
        pthread_mutex_unlock(&g_pool.lk);
        size_t parts = bytes / POOL_MIN_SLICE;
        if (parts > helpers + 1) parts = helpers + 1;
        const size_t slice = ((bytes + parts - 1) / parts + 4095) & ~(size_t)4095;
        own = slice < bytes ? slice : bytes;
        if (own < bytes) pool_submit(&pending, d + own, s ? s + own : NULL, bytes - own, slice);
    }
    if (own) { const struct ptask t = { d, s, own, NULL }; ptask_run(&t); }
    if (own < bytes) pool_wait(&pending);
}

/* ------------------------------------------------------------------------------------------
 * pinned memory for callers
 * ---------------------------------------------------------------------------------------- */

/* Page-locked host memory: buffers from here are used in place by the host-pointer entry points (no staging copy).
 * NULL when the allocation fails.  Freed by eddsa_amd_host_free only. */
void *eddsa_amd_host_alloc(size_t bytes)
{
    struct call c;
    void *p = NULL;
    if (enter(&c, -1)) return NULL;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { hip_forget_error(); p = NULL; }
    leave(&c);
    return p;
}

void eddsa_amd_host_free(void *p)
{
    if (p) HIP_NOTE(hipHostFree(p));
}

/* is [p, p + bytes) page-locked memory the DMA engines can read directly?  BOTH ends are asked (an array whose head was
 * registered and whose tail is pageable - a view that runs past a registered window - is staged like ordinary memory);
 * the runtime has no query for "one allocation", so a range glued together from two registrations passes: each of its
 * pages is page-locked, which is what the copy needs */
static int is_pinned(const void *p, size_t bytes)
{
    hipPointerAttribute_t a, b;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { hip_forget_error(); return 0; }   /* "not registered" is an answer, not a failure */
    if (a.type != hipMemoryTypeHost) return 0;
    if (bytes <= 1) return 1;
    if (hipPointerGetAttributes(&b, (const uint8_t *)p + bytes - 1) != hipSuccess) { hip_forget_error(); return 0; }
    return b.type == hipMemoryTypeHost;
}

/* ------------------------------------------------------------------------------------------
 * the pipeline
 * ---------------------------------------------------------------------------------------- */

#define PIPE_FIRST_CHUNK ((size_t)1 << 17)   /* the first chunk of a call (512 blocks: the chip is full 0.3 ms after the call); later ones double up to the job's stage size */
#define PIPE_CHUNK ((size_t)1 << 18)         /* stage size: 1024 blocks of 256 lanes */
#define PIPE_PIECE ((size_t)8 << 20)         /* staging granularity: a piece is handed to the DMA engine while the next is copied */
#define PIN_CHECK_MIN ((size_t)1 << 20)      /* smaller arrays are staged without asking whether they are pinned */

/* (set by the measurement aids at the end of the file, which only libeddsa_amd_debug.so has) */
static size_t g_pipe_first, g_pipe_stage;   /* eddsa_amd_set_pipeline: 0 = the defaults above / the job's own stage size */
static int g_pipe_chain = -1;               /* -1: the job's own; 0: the lanes' kernels run side by side; 1: in chunk order; 2: verify's next chunk starts beside the main kernel */

enum { WIPE_NONE = 0, WIPE_IN0 = 1, WIPE_OUT = 2 };   /* which staging buffers held secrets */
/* combiner slots (engine.h: COMB_KINDS): small calls of one kind may be merged; KIND_NONE: never */
enum { KIND_NONE = 0, KIND_VERIFY = 1, KIND_SIGN = 2, KIND_X25519 = 3, KIND_GENPUB = 4, KIND_XBASE = 5, KIND_PK_TO_X = 6, KIND_SK_TO_X = 7 };

/* one chunk of a job as its kernels see it: the HBM buffers of the lane that carries it, m items, on stream st */
struct chunk {
    uint8_t *d_out; uint8_t *const *d_in; const uint8_t *d_msgs; size_t m; hipStream_t st;
    const uint64_t *d_off;                     /* ragged messages: the chunk's offset table, rebased to its first byte; else NULL */
    hipEvent_t kdone;                          /* the lane's "kernels queued" event */
    uint32_t *d_stats;                         /* rlc: the pass statistics in HBM (4 words) or NULL */
};

/* what an operation is; the table (g_ops) stands in front of the entry points */
struct hjob;
struct op {
    int n_in; size_t in_w[PIPE_MAX_IN];        /* fixed-width inputs (width 0: the call's own, hjob.stride) */
    size_t out_w; int has_msgs;
    int (*run)(struct engine *e, const struct hjob *j, const struct chunk *c);
    int wipe;                                  /* WIPE_* */
    int chain;                                 /* the kernels of consecutive chunks run in chunk order (else side by side) */
    int kind;                                  /* KIND_*: small calls of this operation may be merged */
    size_t chunk;                              /* items per pipeline stage (0: PIPE_CHUNK) */
    size_t first_chunk;                        /* items of the first chunk (0: PIPE_FIRST_CHUNK); later ones double up to `chunk` */
    int reports;                               /* its kernels report through the engine's status word (take_async_error) */
};

/* a call: the operation and its pointers */
struct hjob {
    const struct op *op;
    const uint8_t *in[PIPE_MAX_IN]; uint8_t *out;
    const uint8_t *msgs; const uint64_t *msg_off; size_t msg_len;
    size_t stride, rec_sig, rec_pub, rec_msg;  /* records: the width of in[0]'s items and the offsets inside them */
    uint32_t *stats;                           /* rlc: host copy of the pass statistics (4 words) or NULL */
    int src_pinned;                            /* every host array of the job is page-locked: no staging */
    const edk_dom *dom;                        /* Ed25519ctx / Ed25519ph: the call's dom2 prefix (lives on msg_call_run's frame); else NULL */
    int digest;                                /* the digest forms: the message slot holds SHA-512(R || A || M), EDDSA_DIGEST_BYTES per item */
    const eddsa_amd_keyset *ks;                /* ed25519_verify_keyed: the caller's key set (in[1] then holds the key indices); else NULL */
    const eddsa_amd_signer *sg;                /* ed25519_sign_keyed: the caller's signer set (in[0] then holds the key indices); else NULL */
};

static size_t in_w(const struct hjob *j, int i) { return j->op->in_w[i] ? j->op->in_w[i] : j->stride; }

/* (new memory starts zeroed, on the stream that will use it: what the allocator hands out is whatever a freed buffer held,
 * and the residue check of the tests - pipe_residue - looks at whole buffers) */
static int dev_grow(void **buf, size_t *cap, size_t need, hipStream_t st)
{
    if (need <= *cap) return 0;
    if (*buf) { wipe_free(*buf, *cap); *buf = NULL; *cap = 0; }
    need = need < 256 ? 256 : need;
    hipError_t e = hipMalloc(buf, need);
    if (e != hipSuccess) return -(int)e;
    e = hipMemsetAsync(*buf, 0, need, st);
    if (e != hipSuccess) { HIP_NOTE(hipFree(*buf)); *buf = NULL; return -(int)e; }
    *cap = need;
    return 0;
}

static void host_free_wiped(void **buf, size_t *cap)
{
    if (*buf) { memset(*buf, 0, *cap); HIP_NOTE(hipHostFree(*buf)); }
    *buf = NULL; *cap = 0;
}

static int host_grow(void **buf, size_t *cap, size_t need)
{
    if (need <= *cap) return 0;
    host_free_wiped(buf, cap);
    need = need < 4096 ? 4096 : need;
    hipError_t e = hipHostMalloc(buf, need, hipHostMallocDefault);
    if (e != hipSuccess) { *buf = NULL; return -(int)e; }
    memset(*buf, 0, need);
    *cap = need;
    return 0;
}

static int pipe_init(struct pipe *p)
{
    int rc = 0;
    if (p->ready) return 0;
    for (int l = 0; l < PIPE_LANES; l++) {
        /* (a call that failed half-way through here is retried by the next one: what exists is kept) */
        if (!p->lane[l].st) TRY(hipStreamCreateWithFlags(&p->lane[l].st, hipStreamNonBlocking));
        if (!p->lane[l].kdone) TRY(hipEventCreateWithFlags(&p->lane[l].kdone, hipEventDisableTiming));
    }
    if (!p->d_stats) TRY(hipMalloc((void **)&p->d_stats, 256));
    if (!p->h_stats) TRY(hipHostMalloc((void **)&p->h_stats, 256, hipHostMallocDefault));
    p->ready = 1;
out:
    return rc;
}

void pipe_setup(struct pipe *p)
{
    pthread_cond_init(&p->lane_cv, NULL);
}

void pipe_release(struct pipe *p)
{
    pthread_cond_destroy(&p->lane_cv);
    for (int l = 0; l < PIPE_LANES; l++) {
        struct lane *L = &p->lane[l];
        for (int i = 0; i < PIPE_MAX_IN; i++) { wipe_free(L->d_in[i], L->d_in_cap[i]); host_free_wiped(&L->h_in[i], &L->h_in_cap[i]); }
        wipe_free(L->d_msgs, 0); host_free_wiped(&L->h_msgs, &L->h_msgs_cap);
        wipe_free(L->d_out, L->d_out_cap); host_free_wiped(&L->h_out, &L->h_out_cap);
        wipe_free(L->d_off, 0); host_free_wiped(&L->h_off, &L->h_off_cap);
        if (L->st) HIP_NOTE(hipStreamDestroy(L->st));
        if (L->kdone) HIP_NOTE(hipEventDestroy(L->kdone));
    }
    if (p->d_stats) HIP_NOTE(hipFree(p->d_stats));
    if (p->h_stats) HIP_NOTE(hipHostFree(p->h_stats));
    memset(p, 0, sizeof(*p));
}

/* Lanes are handed out under pipe_lk and owned through their busy marks, so that the lock is never held while work
 * runs: a call of ONE chunk takes any free lane - three such calls (the combined launches of three operations, say)
 * are in flight side by side -, a call of several chunks takes all three; while one of those waits, no new one-chunk
 * call starts.  Returns the first lane of the job (0 when it has them all), or a negative error. */
static int lanes_acquire(struct engine *e, int all)
{
    struct pipe *p = &e->pipe;
    int got = -1;
    pthread_mutex_lock(&e->pipe_lk);
    int rc = pipe_init(p);
    if (rc) { pthread_mutex_unlock(&e->pipe_lk); return rc; }
    if (all) {
        p->big_waiting++;
        while (p->lane[0].busy || p->lane[1].busy || p->lane[2].busy) pthread_cond_wait(&p->lane_cv, &e->pipe_lk);
        p->big_waiting--;
        for (int l = 0; l < PIPE_LANES; l++) p->lane[l].busy = 1;
        got = 0;
    } else {
        for (;;) {
            for (int l = 0; l < PIPE_LANES && got < 0 && !p->big_waiting; l++) if (!p->lane[l].busy) got = l;
            if (got >= 0) break;
            pthread_cond_wait(&p->lane_cv, &e->pipe_lk);
        }
        p->lane[got].busy = 1;
    }
    pthread_mutex_unlock(&e->pipe_lk);
    return got;
}

static void lanes_release(struct engine *e, int all, int first)
{
    pthread_mutex_lock(&e->pipe_lk);
    for (int l = 0; l < PIPE_LANES; l++) if (all || l == first) e->pipe.lane[l].busy = 0;
    pthread_cond_broadcast(&e->pipe.lane_cv);
    pthread_mutex_unlock(&e->pipe_lk);
}

int pipe_residue(struct engine *e, uint64_t *in0, uint64_t *out)
{
    int rc = lanes_acquire(e, 1);                  /* no job in flight while the buffers are read */
    if (rc < 0) return rc;
    rc = 0;
    for (int l = 0; l < PIPE_LANES && !rc; l++) {
        const struct lane *L = &e->pipe.lane[l];
        rc = count_nonzero_dev(L->d_in[0], L->d_in_cap[0], in0);
        if (!rc) rc = count_nonzero_dev(L->d_out, L->d_out_cap, out);
        for (size_t k = 0; L->h_in[0] && k < L->h_in_cap[0]; k++) *in0 += ((const uint8_t *)L->h_in[0])[k] != 0;
        for (size_t k = 0; L->h_out && k < L->h_out_cap; k++) *out += ((const uint8_t *)L->h_out)[k] != 0;
    }
    lanes_release(e, 1, 0);
    pthread_mutex_lock(&e->comb_q.lk);
    for (int c = 0; c < COMB_KINDS; c++) {
        const struct comb_kind *K = &e->comb_q.kind[c];
        for (size_t k = 0; K->h_in[0] && k < K->h_in_cap[0]; k++) *in0 += ((const uint8_t *)K->h_in[0])[k] != 0;
    }
    pthread_mutex_unlock(&e->comb_q.lk);
    return rc;
}

/* host -> HBM on the lane's stream: staged through *hbuf piece by piece, or straight from page-locked memory */
static int lane_upload(struct lane *L, void *dst, void **hbuf, size_t *hcap, const uint8_t *src, size_t bytes, int staged)
{
    int rc = 0;
    if (!bytes) return 0;
    if (!staged) { TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, L->st)); return 0; }
    if ((rc = host_grow(hbuf, hcap, bytes))) return rc;
    for (size_t off = 0; off < bytes; off += PIPE_PIECE) {
        const size_t pb = bytes - off < PIPE_PIECE ? bytes - off : PIPE_PIECE;
        par_copy((uint8_t *)*hbuf + off, src + off, pb);
        TRY(hipMemcpyAsync((uint8_t *)dst + off, (uint8_t *)*hbuf + off, pb, hipMemcpyHostToDevice, L->st));
    }
out:
    return rc;
}

/* queue the download of the lane's chunk - into pend_via or straight into pend_dst - and the wipe of secret results in HBM */
static int lane_download(struct lane *L, int wipe)
{
    hipError_t e = hipMemcpyAsync(L->pend_via ? L->pend_via : (void *)L->pend_dst, L->pend_dev, L->pend_bytes, hipMemcpyDeviceToHost, L->st);
    if (e == hipSuccess && (wipe & WIPE_OUT)) e = hipMemsetAsync(L->pend_dev, 0, L->pend_bytes, L->st);    /* shared secrets leave HBM with the call */
    L->pend_queued = 1;
    return -(int)e;
}

/* Wait for the kernels of the chunk the lane carries, fetch its results, deliver them and zero the staging copies of
 * secrets.  The download is queued only now, when it can run at once: a copy queued behind kernels still to run sits at
 * the head of one of the DMA engines' queues, and the UPLOADS that the runtime later hands to the same engine wait
 * behind it (measured: the last two pieces of a chunk's upload ran 5 ms late, the whole call 12.4 instead of 10 ms). */
static int lane_drain(struct lane *L, int wipe, int *wipes)
{
    int rc = 0;
    TRY(hipStreamSynchronize(L->st));
    if (L->pend_bytes) {
        if (!L->pend_queued) {
            if ((rc = lane_download(L, wipe))) goto out;
            TRY(hipStreamSynchronize(L->st));
        }
        if (L->pend_via) par_copy(L->pend_dst, L->pend_via, L->pend_bytes);
    }
    /* wipes == NULL: the lane is about to be reused, zero it now; otherwise queue the zeroing (end of the call) */
    if ((wipe & WIPE_IN0) && L->used_in0) { if (wipes) pool_submit(wipes, (uint8_t *)L->h_in[0], NULL, L->used_in0, 0); else par_copy(L->h_in[0], NULL, L->used_in0); }
    if ((wipe & WIPE_OUT) && L->pend_bytes && L->pend_via) { if (wipes) pool_submit(wipes, (uint8_t *)L->pend_via, NULL, L->pend_bytes, 0); else par_copy(L->pend_via, NULL, L->pend_bytes); }
out:
    L->pend_bytes = 0;
    L->used_in0 = 0;
    return rc;
}

static int g_fail_next_host_call;      /* eddsa_amd_debug_fail_next_host_call: set and consumed atomically */

static int64_t now_ns(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (int64_t)ts.tv_sec * 1000000000 + ts.tv_nsec;
}

/* measurement aid: host-side time stamps of the last host-pointer call (eddsa_amd_debug_pipe_trace) */
#define TRACE_MAX 512
/* one trace per process; stamps of concurrent calls interleave.  Slots are reserved atomically (leaders of different
 * operations stamp at the same time) and filled with atomic stores (a call that restarts the trace may hand a slot out
 * again while its previous owner is still writing: the stamp is then a mix of two calls' - it is a diagnostic - but never a
 * data race); on / n / seen are read and written atomically; the reader holds g_table for writing, i.e. no call is in flight */
static struct { int on, n, seen; int tag[TRACE_MAX]; unsigned chunk[TRACE_MAX]; int64_t t_ns[TRACE_MAX]; } g_trace;
#define TRACE_ON() __atomic_load_n(&g_trace.on, __ATOMIC_RELAXED)
#define TRACE(tag_, k_) do { if (TRACE_ON()) { const int i_ = __atomic_fetch_add(&g_trace.n, 1, __ATOMIC_RELAXED); \
    if (i_ >= 0 && i_ < TRACE_MAX) { __atomic_store_n(&g_trace.tag[i_], (tag_), __ATOMIC_RELAXED); \
        __atomic_store_n(&g_trace.chunk[i_], (unsigned)(k_), __ATOMIC_RELAXED); __atomic_store_n(&g_trace.t_ns[i_], now_ns(), __ATOMIC_RELAXED); } } } while (0)
#define TRACE_RESTART() __atomic_store_n(&g_trace.n, 0, __ATOMIC_RELAXED)

/* A ragged call's offset table (m + 1 entries of the caller's memory) must not decrease, and the bytes it spans must be an
 * amount a buffer can hold: everything below takes msg_off[k + 1] - msg_off[k] for a length.  Checked chunk by chunk, right
 * before the chunk's offsets are first used (the walk of chunk k runs beside the GPU work of chunk k - 1); a table that
 * fails ends the call with -hipErrorInvalidValue before a byte of that chunk is read. */
#define MSG_BYTES_MAX ((uint64_t)1 << 46)
static int offsets_ok(const uint64_t *off, size_t m)
{
    uint64_t bad = 0;
    for (size_t t = 0; t < m; t++) bad |= (uint64_t)(off[t + 1] < off[t]);
    return !bad && off[m] - off[0] <= MSG_BYTES_MAX;
}

/* dst[0 .. m] = the offset table off[0 .. m], rebased to 0 */
static void offsets_rebase(uint64_t *dst, const uint64_t *off, size_t m)
{
    const uint64_t base0 = off[0];
    for (size_t t = 0; t <= m; t++) dst[t] = off[t] - base0;
}

/* one host-pointer call in flight: the job, how it is cut into chunks, its lanes and which of its arrays are staged */
struct pcall {
    struct engine *e; const struct hjob *j; size_t n;
    int ragged;                                /* the messages come with an offset table */
    size_t first, stage;                       /* items of the first chunk and of a full stage */
    int all, base;                             /* the call holds all lanes; else the one lane it holds */
    int staged_in[PIPE_MAX_IN], staged_msgs, staged_out;   /* 0: the caller's array is page-locked and used in place */
    int wipes;                                 /* zeroing of pinned staging buffers queued with the copier pool (pool_wait) */
};

/* chunk k travels on lane k mod 3 (a call of one chunk: on the lane it was given) */
static struct lane *call_lane(const struct pcall *c, unsigned k) { return &c->e->pipe.lane[c->all ? k % PIPE_LANES : (unsigned)c->base]; }

/* items of chunk k, `left` items being still to do: the first chunk doubles up to the stage size */
static size_t chunk_items(const struct pcall *c, unsigned k, size_t left)
{
    size_t m = c->first << (k < 8 ? k : 8);
    if (m > c->stage) m = c->stage;
    return !c->all || m > left || left - m < m / 2 ? left : m;   /* (a short tail travels with the last chunk) */
}

/* stage and upload items lo .. lo + m of the call on lane L: inputs, message bytes, offset table; room for the output */
static int chunk_upload(const struct pcall *c, struct lane *L, size_t lo, size_t m)
{
    const struct hjob *j = c->j;
    int rc = 0;
    for (int i = 0; i < j->op->n_in; i++) {
        if ((rc = dev_grow(&L->d_in[i], &L->d_in_cap[i], m * in_w(j, i), L->st))) goto out;
        if ((rc = lane_upload(L, L->d_in[i], &L->h_in[i], &L->h_in_cap[i], j->in[i] + lo * in_w(j, i), m * in_w(j, i), c->staged_in[i]))) goto out;
    }
    if (c->staged_in[0]) L->used_in0 = m * in_w(j, 0);
    if (j->op->has_msgs) {
        /* ragged messages: the chunk's own bytes, msg_off[lo] .. msg_off[lo + m) */
        const size_t bytes = c->ragged ? (size_t)(j->msg_off[lo + m] - j->msg_off[lo]) : m * j->msg_len;
        const uint8_t *src = c->ragged ? j->msgs + j->msg_off[lo] : j->msgs + lo * j->msg_len;
        if ((rc = dev_grow(&L->d_msgs, &L->d_msgs_cap, bytes, L->st))) goto out;
        if ((rc = lane_upload(L, L->d_msgs, &L->h_msgs, &L->h_msgs_cap, src, bytes, c->staged_msgs))) goto out;
    }
    if (c->ragged) {
        /* ... and its own offset table, rebased to the chunk's first byte (the kernels index it by the item's
         * number inside the chunk).  A table that starts at 0 in page-locked memory - the combiner's - goes as it is. */
        const size_t ob = (m + 1) * sizeof(uint64_t);
        const int as_it_is = j->src_pinned && j->msg_off[lo] == 0;
        if ((rc = dev_grow(&L->d_off, &L->d_off_cap, ob, L->st))) goto out;
        if (!as_it_is && (rc = host_grow(&L->h_off, &L->h_off_cap, ob))) goto out;
        if (!as_it_is) offsets_rebase((uint64_t *)L->h_off, j->msg_off + lo, m);
        TRY(hipMemcpyAsync(L->d_off, as_it_is ? (const void *)(j->msg_off + lo) : L->h_off, ob, hipMemcpyHostToDevice, L->st));
    }
    rc = dev_grow(&L->d_out, &L->d_out_cap, m * j->op->out_w, L->st);
out:
    return rc;
}

/* queue the kernels of chunk k (m items, on lane L) - behind those of the chunk before it, on lane `prev`, where chunks run in order */
static int chunk_launch(const struct pcall *c, struct lane *L, const struct lane *prev, unsigned k, size_t m)
{
    const struct hjob *j = c->j;
    int rc = 0;
    if (prev && (g_pipe_chain < 0 ? j->op->chain : g_pipe_chain)) TRY(hipStreamWaitEvent(L->st, prev->kdone, 0));      /* kernels in chunk order */
    const struct chunk ch = { .d_out = (uint8_t *)L->d_out, .d_in = (uint8_t *const *)L->d_in, .d_msgs = (const uint8_t *)L->d_msgs, .m = m, .st = L->st,
                              .d_off = c->ragged ? (const uint64_t *)L->d_off : NULL, .kdone = L->kdone, .d_stats = j->stats ? c->e->pipe.d_stats : NULL };
    rc = j->op->run(c->e, j, &ch);
    TRACE(3, k);
    if (!rc && __atomic_exchange_n(&g_fail_next_host_call, 0, __ATOMIC_ACQ_REL)) rc = -(int)hipErrorUnknown;
out:
    return rc;
}

/* note where the results of the chunk on lane L (items lo .. lo + m) go: the download is queued by lane_drain, once the
 * kernels are done - except for a call of one chunk, which has no uploads to hold up: everything in order, one wait */
static int chunk_note_download(const struct pcall *c, struct lane *L, size_t lo, size_t m)
{
    const struct hjob *j = c->j;
    int rc = 0;
    L->pend_via = NULL;
    if (c->staged_out) {
        if ((rc = host_grow(&L->h_out, &L->h_out_cap, m * j->op->out_w))) return rc;
        L->pend_via = (uint8_t *)L->h_out;
    }
    L->pend_dst = j->out + lo * j->op->out_w; L->pend_dev = (uint8_t *)L->d_out; L->pend_bytes = m * j->op->out_w;
    L->pend_queued = 0;
    if (lo == 0 && m == c->n) rc = lane_download(L, j->op->wipe);
    return rc;
}

/* the chunks of the call, one after the other; on return without an error every lane of the call is drained */
static int call_chunks(struct pcall *c)
{
    const struct hjob *j = c->j;
    const int wipe = j->op->wipe;
    struct lane *prev = NULL;
    int rc = 0;
    size_t lo = 0;
    for (unsigned k = 0; lo < c->n; k++) {
        struct lane *L = call_lane(c, k);
        const size_t m = chunk_items(c, k, c->n - lo);
        if (c->ragged && !offsets_ok(j->msg_off + lo, m)) return -(int)hipErrorInvalidValue;   /* before anything of the chunk is staged */
        /* the lane's previous chunk (k - 3): the two chunks after it keep the GPU busy meanwhile */
        if (k >= PIPE_LANES && (rc = lane_drain(L, wipe, NULL))) goto out;    /* (every call leaves its lanes drained) */
        TRACE(1, k);
        if ((rc = chunk_upload(c, L, lo, m))) goto out;
        TRACE(2, k);
        rc = chunk_launch(c, L, prev, k, m);
        prev = L;
        if (rc || (rc = chunk_note_download(c, L, lo, m))) goto out;
        /* secrets do not outlive the call in HBM */
        if (wipe & WIPE_IN0) TRY(hipMemsetAsync(L->d_in[0], 0, m * in_w(j, 0), L->st));
        lo += m;
        TRACE(4, k);
        if (lo >= c->n) {                  /* the chunks still in flight, oldest first */
            for (unsigned t = k + 1 < PIPE_LANES ? PIPE_LANES - k : 1; t <= PIPE_LANES; t++)
                if ((rc = lane_drain(call_lane(c, k + t), wipe, &c->wipes))) goto out;
            TRACE(5, k);
        }
    }
out:
    return rc;
}

/* a failed call must not leave its secrets behind either (best effort: whole buffers, HBM and pinned) */
static void call_scrub(struct pcall *c)
{
    const int wipe = c->j->op->wipe;
    for (int l = 0; l < PIPE_LANES; l++) {
        struct lane *L = &c->e->pipe.lane[l];
        if (!c->all && l != c->base) continue;
        HIP_NOTE(hipStreamSynchronize(L->st));
        L->pend_bytes = 0; L->used_in0 = 0;
        if ((wipe & WIPE_IN0) && L->d_in[0]) HIP_NOTE(hipMemsetAsync(L->d_in[0], 0, L->d_in_cap[0], L->st));
        if ((wipe & WIPE_OUT) && L->d_out) HIP_NOTE(hipMemsetAsync(L->d_out, 0, L->d_out_cap, L->st));
        if (wipe) HIP_NOTE(hipStreamSynchronize(L->st));
        if ((wipe & WIPE_IN0) && L->h_in[0]) pool_submit(&c->wipes, (uint8_t *)L->h_in[0], NULL, L->h_in_cap[0], 0);
        if ((wipe & WIPE_OUT) && L->h_out) pool_submit(&c->wipes, (uint8_t *)L->h_out, NULL, L->h_out_cap, 0);
    }
}

/* One host-pointer job on engine e (its device is current).
 * Chunk k travels on lane k mod 3: [wait for the lane's previous chunk, fetch and deliver its results] - stage and
 * upload - kernels, all on the lane's stream; copies and kernels of different lanes overlap.  How the KERNELS of
 * consecutive chunks are ordered is the operation's choice (op.chain; tools/pipe_sweep.py has the measurements):
 *   in chunk order (each chunk's kernels wait for the previous lane's `kdone`): x25519, sign and the other fixed-base
 *     operations, whose chunk is one long kernel - side by side three of them share the chip, finish together, and the
 *     pipeline drains and refills in bursts (x25519 84-93 M/s against 103-105 in order);
 *   side by side: verify, whose three kernels per chunk leave ramps and tails that the neighbours fill (95.7 M/s
 *     against 79-86 in order).
 * `kdone` is recorded before a verify pass waits for its exact path, so that those few latency-bound waves never hold
 * up the next chunk (each lane's stream has its own workspace).
 * traced: the caller (the combiner's leader) has started the call's trace already. */
static int pipe_run_on(struct engine *e, const struct hjob *j, size_t n, int traced)
{
    struct pipe *p = &e->pipe;
    int rc = 0;
    if (n == 0) return 0;
    struct pcall c = { .e = e, .j = j, .n = n, .ragged = j->op->has_msgs && j->msg_off != NULL };
    const int tunable = j->stats == NULL;                       /* (a combination covers a fixed number of items) */
    c.stage = tunable && g_pipe_stage ? g_pipe_stage : j->op->chunk ? j->op->chunk : PIPE_CHUNK;
    c.first = tunable && g_pipe_first ? g_pipe_first : j->op->first_chunk ? j->op->first_chunk : PIPE_FIRST_CHUNK;
    /* The offset table as a whole, before anything is touched: it must not end before it starts, nor span more than 2^46
     * bytes (include/eddsa_amd.h).  Whether it DEcreases somewhere in between is checked chunk by chunk (call_chunks), as each
     * chunk is about to be staged (one pass over the table in step with the copies instead of a second one in front of them): a
     * table that is bad further on is found after earlier chunks have run, the call then returns -hipErrorInvalidValue and its
     * outputs are unspecified, as on every error. */
    if (c.ragged && (j->msg_off[n] < j->msg_off[0] || j->msg_off[n] - j->msg_off[0] > MSG_BYTES_MAX)) return -(int)hipErrorInvalidValue;
    /* one chunk, one lane (any); several chunks - and the batch verification, whose statistics live in the pipe - all of them */
    c.all = j->stats != NULL || n > c.first;
    c.base = lanes_acquire(e, c.all);
    if (c.base < 0) return c.base;
    if (TRACE_ON() && !traced) TRACE_RESTART();
    TRACE(0, 0);
    /* which of the call's arrays go through pinned staging: all, unless the array is large enough to ask and page-locked */
    const size_t msg_total = !j->op->has_msgs ? 0 : c.ragged ? (size_t)(j->msg_off[n] - j->msg_off[0]) : n * j->msg_len;
    for (int i = 0; i < j->op->n_in; i++)
        c.staged_in[i] = !j->src_pinned && !(n * in_w(j, i) >= PIN_CHECK_MIN && is_pinned(j->in[i], n * in_w(j, i)));
    c.staged_msgs = !j->src_pinned && !(msg_total >= PIN_CHECK_MIN && is_pinned(c.ragged ? j->msgs + j->msg_off[0] : j->msgs, msg_total));
    c.staged_out = !j->src_pinned && !(n * j->op->out_w >= PIN_CHECK_MIN && is_pinned(j->out, n * j->op->out_w));
    if (j->stats) {
        TRY(hipMemsetAsync(p->d_stats, 0, 16, p->lane[0].st));
        TRY(hipStreamSynchronize(p->lane[0].st));           /* the other lanes' kernels add to it too */
    }
    if ((rc = call_chunks(&c))) goto out;
    if (j->stats) {
        TRY(hipMemcpyAsync(p->h_stats, p->d_stats, 16, hipMemcpyDeviceToHost, p->lane[0].st));
        TRY(hipStreamSynchronize(p->lane[0].st));
        memcpy(j->stats, p->h_stats, 16);
    }
    /* every lane of the call has been waited for: what a verify pass's kernels reported (a hand-off given up) is this
     * call's error (the other operations' kernels have nothing to report: a sign call does not take a verify call's word) */
    if (j->op->reports) rc = take_async_error(e);
out:
    if (rc) call_scrub(&c);
    if (j->op->wipe) pool_wait(&c.wipes);      /* nothing secret outlives the call in the pinned staging buffers */
    TRACE(6, 0);
    lanes_release(e, c.all, c.base);
    return rc;
}

/* ------------------------------------------------------------------------------------------
 * the combiner: concurrent small calls of one operation become one launch
 * ---------------------------------------------------------------------------------------- */

#define COMBINE_MAX_N 64                     /* items of a call that may be merged */
#define COMBINE_MAX_BYTES ((size_t)1 << 20)  /* ... and its message bytes */
#define COMBINE_MAX_BATCH 16384              /* items per combined launch */
#define COMBINE_MAX_BATCH_BYTES ((size_t)64 << 20)   /* ... and its message bytes (pinned staging of the packed batch) */
#define COMBINE_RETRY_GIVE_UP 4               /* request-by-request retries of a failed launch that may fail alike in a row before the rest are given the launch's error */
#define COMBINE_GATHER_NS 80000              /* how long a leader elected under contention waits for the callers of the previous batch */

struct creq { const struct hjob *j; size_t n; int rc, done; struct creq *next; };

void combiner_init(struct combiner *q)
{
    memset(q, 0, sizeof(*q));
    pthread_mutex_init(&q->lk, NULL);
}

void combiner_release(struct combiner *q)
{
    for (int c = 0; c < COMB_KINDS; c++) {
        struct comb_kind *K = &q->kind[c];
        for (int i = 0; i < PIPE_MAX_IN; i++) host_free_wiped(&K->h_in[i], &K->h_in_cap[i]);
        host_free_wiped(&K->h_msgs, &K->h_msgs_cap);
        host_free_wiped(&K->h_out, &K->h_out_cap);
        { void *p = K->h_off; size_t cap = K->h_off_cap; host_free_wiped(&p, &cap); K->h_off = NULL; K->h_off_cap = 0; }
    }
    pthread_mutex_destroy(&q->lk);
}

/* the leader's work: pack the requests of `batch` (a list through ->next, all of one operation), run them as one job
 * from the operation's pinned buffers, scatter the results.  Returns the job's status. */
static int combiner_run(struct engine *e, struct comb_kind *K, struct creq *batch, size_t total)
{
    const struct hjob *j0 = batch->j;
    const struct op *op = j0->op;
    int rc = 0, same_len = 1;
    size_t msg_bytes = 0;
    for (struct creq *r = batch; r; r = r->next) {
        if (r->j->msg_len != j0->msg_len) same_len = 0;
        msg_bytes += r->n * r->j->msg_len;
    }
    for (int i = 0; i < op->n_in; i++) if ((rc = host_grow(&K->h_in[i], &K->h_in_cap[i], total * op->in_w[i]))) return rc;
    if (op->has_msgs && (rc = host_grow(&K->h_msgs, &K->h_msgs_cap, msg_bytes))) return rc;
    if ((rc = host_grow(&K->h_out, &K->h_out_cap, total * op->out_w))) return rc;
    if (op->has_msgs && !same_len) {
        void *p = K->h_off;
        rc = host_grow(&p, &K->h_off_cap, (total + 1) * sizeof(uint64_t));
        K->h_off = (uint64_t *)p;
        if (rc) return rc;
    }
    size_t at = 0, mat = 0;
    for (struct creq *r = batch; r; r = r->next) {
        for (int i = 0; i < op->n_in; i++) memcpy((uint8_t *)K->h_in[i] + at * op->in_w[i], r->j->in[i], r->n * op->in_w[i]);
        if (op->has_msgs) {
            if (r->n * r->j->msg_len != 0) memcpy((uint8_t *)K->h_msgs + mat, r->j->msgs, r->n * r->j->msg_len);
            if (!same_len) for (size_t k = 0; k < r->n; k++) K->h_off[at + k] = mat + k * r->j->msg_len;
            mat += r->n * r->j->msg_len;
        }
        at += r->n;
    }
    if (op->has_msgs && !same_len) K->h_off[total] = mat;
    struct hjob big = *j0;
    for (int i = 0; i < op->n_in; i++) big.in[i] = (const uint8_t *)K->h_in[i];
    big.msgs = (const uint8_t *)K->h_msgs;
    big.msg_off = op->has_msgs && !same_len ? K->h_off : NULL;
    big.out = (uint8_t *)K->h_out;
    big.src_pinned = 1;
    TRACE(9, (unsigned)total);
    rc = pipe_run_on(e, &big, total, 1);
    at = 0;
    for (struct creq *r = batch; r && !rc; r = r->next) {
        memcpy(r->j->out, (uint8_t *)K->h_out + at * op->out_w, r->n * op->out_w);
        at += r->n;
    }
    /* the packed copies of secrets go as well */
    if (op->wipe & WIPE_IN0) memset(K->h_in[0], 0, total * op->in_w[0]);
    if (op->wipe & WIPE_OUT) memset(K->h_out, 0, total * op->out_w);
    TRACE(10, (unsigned)total);
    if (TRACE_ON() == 2 && total >= 32 && __atomic_add_fetch(&g_trace.seen, 1, __ATOMIC_RELAXED) == 20)
        __atomic_store_n(&g_trace.on, 0, __ATOMIC_RELAXED);   /* on = 2: keep the 20th launch that carried 32 calls or more */
    return rc;
}

/* Waiters sleep on their operation's generation counter (one per operation: with one for all, every completion woke
 * the callers of the other operations too - 256 threads split over four operations spent their time being woken for
 * nothing, 38-80 k calls/s), not on a condition variable: when a launch completes, every
 * caller it carried is woken at once and leaves on its own `done` flag without touching the queue's mutex (with a
 * condition variable the 64 callers of a launch re-acquired the mutex one after the other, a context switch each,
 * which cost more than the GPU pass). */
static void gen_wait(uint32_t *gen, uint32_t seen) { (void)syscall(SYS_futex, gen, FUTEX_WAIT_PRIVATE, seen, NULL, NULL, 0); }
static void gen_wake_all(uint32_t *gen) { (void)syscall(SYS_futex, gen, FUTEX_WAKE_PRIVATE, INT_MAX, NULL, NULL, 0); }

/* Under contention the callers of the launch that has just finished are about to queue again (they do within
 * microseconds of being woken): give them a moment, or the callers split into two camps that take turns and
 * every launch carries half of them.  Expected: whoever was already waiting when that launch ended, plus the
 * calls it carried.  Never long; a lone caller (the previous launch carried one call) never waits.
 * Entered and left with q->lk held; while the leader yields, the lock is dropped so that the callers can queue. */
static void leader_gather(struct combiner *q, const struct comb_kind *K)
{
    const unsigned want = K->waiting_at_end + K->last_reqs;
    if (K->last_reqs <= 1 || K->queued >= want) return;
    const int64_t until = now_ns() + COMBINE_GATHER_NS;
    pthread_mutex_unlock(&q->lk);
    for (;;) {
        sched_yield();
        pthread_mutex_lock(&q->lk);
        if (K->queued >= want || now_ns() >= until) break;
        pthread_mutex_unlock(&q->lk);
    }
}

/* Take everything queued for operation `kind` off the queue, up to the limits of one launch (the leader's own request is
 * among it unless thousands are ahead of it: then it leads again): a list through ->next.  Entered and left with q->lk held. */
static struct creq *batch_unlink(struct combiner *q, struct comb_kind *K, int kind, size_t *total, size_t *reqs)
{
    struct creq *batch = NULL, *btail = NULL, **pp = &q->head, *last = NULL;
    size_t bytes = 0;
    *total = *reqs = 0;
    while (*pp) {
        struct creq *r = *pp;
        const size_t rb = r->j->op->has_msgs ? r->n * r->j->msg_len : 0;
        if (r->j->op->kind == kind && *total + r->n <= COMBINE_MAX_BATCH && (*reqs == 0 || bytes + rb <= COMBINE_MAX_BATCH_BYTES)) {
            *pp = r->next;
            r->next = NULL;
            if (btail) btail->next = r; else batch = r;
            btail = r;
            *total += r->n; ++*reqs; bytes += rb;
            K->queued--;
        } else { last = r; pp = &r->next; }
    }
    q->tail = last;
    return batch;
}

/* A merged launch shares one status, and the eddsa.h callers abort() on failure: before anybody is told, every
 * request gets a run of its own (a transient error, or the packed batch's staging allocation, need not concern
 * the others; a request that is itself the cause fails again, alone) */
/* ... but not without end: a batch holds up to 16 384 requests, and when the cause is the device (lost, out of
 * memory) every retry stages secrets, fails, waits and wipes while all callers stay blocked.  After
 * COMBINE_RETRY_GIVE_UP retries in a row that end with the batch's own error the rest are told that error. */
/* Only for errors of the DEVICE: an error a caller can bring about by itself (an invalid argument, a bad offset
 * table) says nothing about the next request - four faulty callers in a row must not fail everybody behind
 * them - so such a batch is retried request by request to the end. */
/* Called without q->lk (no lock is held while a job runs); every r->rc of the batch holds rc, the launch's error. */
static void batch_retry(struct engine *e, struct creq *batch, int rc)
{
    const int device_fault = rc != -(int)hipErrorInvalidValue && rc != -(int)hipErrorInvalidDevicePointer;
    int same = 0;
    for (struct creq *r = batch; r; r = r->next) {
        if (device_fault && same >= COMBINE_RETRY_GIVE_UP) continue;
        r->rc = pipe_run_on(e, r->j, r->n, 1);
        same = r->rc == rc ? same + 1 : 0;
    }
}

/* Hand the batch's results to its callers and wake them.  Entered and left without q->lk, which it takes for the bookkeeping. */
static void batch_publish(struct combiner *q, struct comb_kind *K, struct creq *batch, size_t reqs)
{
    pthread_mutex_lock(&q->lk);
    q->batches++; q->items += reqs;
    K->last_reqs = (unsigned)reqs;
    K->waiting_at_end = K->queued;
    for (struct creq *r = batch, *nx; r; r = nx) {  /* a caller may return (and its request vanish) the moment `done` is set */
        nx = r->next;
        __atomic_store_n(&r->done, 1, __ATOMIC_RELEASE);
    }
    K->active = 0;
    __atomic_add_fetch(&K->gen, 1, __ATOMIC_RELEASE);
    pthread_mutex_unlock(&q->lk);
    gen_wake_all(&K->gen);
}

/* One leader per OPERATION at a time: the calls queued for verify travel in one launch while, side by side on another
 * lane of the pipeline, the calls queued for sign travel in theirs (threads that issue different operations would
 * otherwise take turns: 64 threads split over four operations got 28 k calls/s that way). */
static int combiner_submit(struct engine *e, const struct hjob *j, size_t n)
{
    struct combiner *q = &e->comb_q;
    struct comb_kind *K = &q->kind[j->op->kind];
    struct creq me = { j, n, 0, 0, NULL };
    pthread_mutex_lock(&q->lk);
    if (q->tail) q->tail->next = &me; else q->head = &me;
    q->tail = &me;
    K->queued++;
    while (!__atomic_load_n(&me.done, __ATOMIC_ACQUIRE)) {    /* (q->lk is held here) */
        if (K->active) {
            const uint32_t seen = __atomic_load_n(&K->gen, __ATOMIC_RELAXED);
            pthread_mutex_unlock(&q->lk);
            gen_wait(&K->gen, seen);                   /* returns at once if a launch of this operation completed in between */
            if (__atomic_load_n(&me.done, __ATOMIC_ACQUIRE)) return me.rc;
            pthread_mutex_lock(&q->lk);
            continue;
        }
        K->active = 1;                                 /* this thread leads one launch */
        if (TRACE_ON()) TRACE_RESTART();
        TRACE(7, 0);
        leader_gather(q, K);
        TRACE(8, K->queued);
        size_t total, reqs;
        struct creq *batch = batch_unlink(q, K, j->op->kind, &total, &reqs);
        pthread_mutex_unlock(&q->lk);                  /* no lock is held while a job runs */
        const int rc = reqs == 1 && batch == &me ? pipe_run_on(e, j, n, 1) : combiner_run(e, K, batch, total);
        for (struct creq *r = batch; r; r = r->next) r->rc = rc;
        if (rc && reqs > 1) batch_retry(e, batch, rc);
        batch_publish(q, K, batch, reqs);
        pthread_mutex_lock(&q->lk);
    }
    pthread_mutex_unlock(&q->lk);
    return me.rc;
}

/* on the default device - a keyed call: on its key set's or its signer set's */
static int pipe_run(const struct hjob j, size_t n)
{
    struct call c;
    if (n == 0) return 0;
    int rc = enter(&c, j.ks ? j.ks->device : j.sg ? j.sg->device : -1);
    if (rc) return rc;
    if (j.op->kind && n <= COMBINE_MAX_N && !(j.op->has_msgs && (j.msg_off || n * j.msg_len > COMBINE_MAX_BYTES)))
        rc = combiner_submit(c.e, &j, n);
    else
        rc = pipe_run_on(c.e, &j, n, 0);
    leave(&c);
    return rc;
}

/* ------------------------------------------------------------------------------------------
 * operations
 * ---------------------------------------------------------------------------------------- */

/* verify: chunks of 2^16, 2^17, 2^18 items, then the rest in one (measured, tools/pipe_verify_sweep.py, 2^20 items from
 * malloc memory, round 4: stage 2^20 98.8 M/s on the config-2 mix and 102.2 on valid signatures, stage 2^19 98.2 / 101.4):
 * the large last chunk hides its exact chain behind a main kernel of several rounds, as one big pass does */
#define PIPE_CHUNK_VERIFY CHUNK_MAX
#define PIPE_FIRST_CHUNK_VERIFY ((size_t)1 << 16)   /* the first chunk of a verify call (the other operations: PIPE_FIRST_CHUNK) */

/* record the lane's "kernels queued" event (verify does it itself, before its stream waits for the exact path) */
static int run_done(int rc, const struct chunk *c) { return !rc && hipEventRecord(c->kdone, c->st) != hipSuccess ? -(int)hipErrorUnknown : rc; }
/* Every verify form: the job says which (engine.h: verify_form - its key set, the digest flag, the dom2 prefix; a job that carries
 * statistics is the combination), the chunk brings the buffers.  Keyed: the chunk's second input is its slice of the key indices.
 * Digests and prehashes travel in the message slot, 64 bytes per item, staged like any fixed-length message. */
static int run_verify(struct engine *e, const struct hjob *j, const struct chunk *c)
{
    const struct verify_form f = { .ks = j->ks, .digest = j->digest, .dom = j->dom, .rlc = j->stats != NULL };
    const edk_verify_src src = j->stride ? verify_src_records(c->d_in[0], j->stride, j->rec_sig, j->rec_pub, j->rec_msg, j->msg_len)
                                         : verify_src(&f, c->d_in[0], c->d_in[1], c->d_msgs, c->d_off, j->msg_len);
    if (f.rlc) return run_done(rlc_on(e, c->d_out, c->d_stats, &src, c->m, c->st), c);
    return verify_on(e, c->d_out, &src, c->m, c->st, c->kdone, g_pipe_chain == 2);
}
/* Every sign form.  Over a signer set (j->sg) the chunk's one input is its slice of the key indices and the secrets come from the
 * set (the lane's second input buffer is not read); j->dom NULL: Ed25519, else Ed25519ctx / Ed25519ph under the call's prefix */
static int run_sign(struct engine *e, const struct hjob *j, const struct chunk *c)
{
    return run_done(sign_on(e, c->d_out, j->sg, c->d_in[0], c->d_in[1], c->d_msgs, c->d_off, j->msg_len, c->m, j->dom, c->st), c);
}
static int run_x25519(struct engine *e, const struct hjob *j, const struct chunk *c)
{
    (void)j;
    return run_done(x25519_on(e, c->d_out, c->d_in[0], c->d_in[1], c->m, c->st), c);
}
/* the operations of one 32-byte input and one 32-byte output */
#define RUN_1IN(name_, on_) static int name_(struct engine *e, const struct hjob *j, const struct chunk *c) \
    { (void)j; return run_done(on_(e, c->d_out, c->d_in[0], c->m, c->st), c); }
RUN_1IN(run_genpub, genpub_on)
RUN_1IN(run_xbase, xbase_on)
RUN_1IN(run_pk_to_x, pk_to_x_on)
RUN_1IN(run_sk_to_x, sk_to_x_on)
RUN_1IN(run_classify, classify_on)                 /* (one byte out, like a verdict) */
/* [m]P + [a]B: the points are input 0; an array the caller left out (mul NULL: m = 1, add NULL: a = 0) is no input at all - nothing
 * is staged or uploaded for it - so the four combinations are four rows, and a row's function says which input is which */
#define RUN_MULADD(name_, mul_, add_) static int name_(struct engine *e, const struct hjob *j, const struct chunk *c) \
    { (void)j; return run_done(muladd_on(e, c->d_out, c->d_in[0], mul_, add_, c->m, c->st), c); }
RUN_MULADD(run_muladd, c->d_in[1], c->d_in[2])
RUN_MULADD(run_muladd_mul, c->d_in[1], NULL)
RUN_MULADD(run_muladd_add, NULL, c->d_in[1])
RUN_MULADD(run_muladd_points, NULL, NULL)

/* The table of operations.  A row says what the pipeline and the combiner need to know of a call: whether small calls may be merged
 * (kind), the widths of its inputs, its chunk sizes, the order of its chunks' kernels and what is wiped - not which form of verify
 * or sign it is; that is the job's (hjob.ks, .digest, .dom, .stats, .sg).
 * Verify - measured (tools/pipe_sweep.py, 2^20 items from malloc memory): the three kernels of a verify chunk leave ramps and tails
 * that the neighbouring chunks' kernels fill when the lanes run side by side (95.7 M/s; in chunk order 79-86), and the small first
 * chunk gets the chip working 0.2 ms after the call.
 *   OP_VERIFY            ed25519_verify_batch[_multi] alone: the one verify row the combiner merges
 *   OP_VERIFY_UNMERGED   the digest forms (their message counterparts with the digests in the message slot) and Ed25519ctx / Ed25519ph
 *                        (two small calls may carry different contexts)
 *   OP_VERIFY_RLC        the batch verification from messages or digests: one combination per 2^20 items
 *   OP_VERIFY_RECORDS    one input of the call's own width
 *   OP_VERIFY_KEYED      every per-item form over a key set (messages, digests, ctx / ph): signatures and 4-byte key indices; never
 *                        merged - two small calls may carry different key sets
 *   OP_VERIFY_KEYED_RLC  the batch verification over a key set: the inputs of OP_VERIFY_KEYED, the chunks of OP_VERIFY_RLC
 *   OP_SIGN              ed25519_sign_batch[_multi] alone: merged
 *   OP_SIGN_UNMERGED     Ed25519ctx / Ed25519ph
 *   OP_SIGN_KEYED        every form over a signer set: 4 bytes of key index per item where the others upload 64 bytes of keys; never
 *                        merged - two small calls may carry different signer sets.  A signing process keeps nothing of a call in the
 *                        staging buffers: which key signed what, and the signatures, are zeroed there like the other operations' secrets
 *   OP_CLASSIFY          ed25519_point_classify_batch: 32 bytes in, one class byte out, nothing secret; never merged
 *   OP_POINT_MULADD      ed25519_point_muladd_batch with both scalar arrays: three 32-byte inputs (points, mul, add), 32 bytes out,
 *                        nothing secret (public keys and public derivation scalars); never merged; a pass is one long chain kernel
 *                        between two short ones, so its chunks run in order like the fixed-base operations'
 *   OP_POINT_MULADD_MUL / _ADD / _POINTS   the same call with add, mul or both NULL: the rows without the absent inputs */
enum { OP_VERIFY, OP_VERIFY_UNMERGED, OP_VERIFY_RLC, OP_VERIFY_RECORDS, OP_VERIFY_KEYED, OP_VERIFY_KEYED_RLC, OP_SIGN, OP_SIGN_UNMERGED, OP_SIGN_KEYED,
       OP_X25519, OP_GENPUB, OP_XBASE, OP_PK_TO_X, OP_SK_TO_X, OP_CLASSIFY, OP_POINT_MULADD, OP_POINT_MULADD_MUL, OP_POINT_MULADD_ADD,
       OP_POINT_MULADD_POINTS };
#define VERIFY_ROW(kind_, w1_, chunk_, first_) { .n_in = 2, .in_w = { 64, w1_, 0 }, .out_w = 1, .has_msgs = 1, .run = run_verify, .wipe = WIPE_NONE, \
    .chain = 0, .kind = kind_, .chunk = chunk_, .first_chunk = first_, .reports = 1 }
static const struct op g_ops[] = {
    [OP_VERIFY] = VERIFY_ROW(KIND_VERIFY, 32, PIPE_CHUNK_VERIFY, PIPE_FIRST_CHUNK_VERIFY),
    [OP_VERIFY_UNMERGED] = VERIFY_ROW(KIND_NONE, 32, PIPE_CHUNK_VERIFY, PIPE_FIRST_CHUNK_VERIFY),
    [OP_VERIFY_RLC] = VERIFY_ROW(KIND_NONE, 32, CHUNK_MAX, CHUNK_MAX),
    [OP_VERIFY_RECORDS] = { .n_in = 1, .in_w = { 0, 0, 0 }, .out_w = 1, .has_msgs = 0, .run = run_verify, .wipe = WIPE_NONE, .chain = 0,
                    .kind = KIND_NONE, .chunk = PIPE_CHUNK_VERIFY, .first_chunk = PIPE_FIRST_CHUNK_VERIFY, .reports = 1 },
    [OP_VERIFY_KEYED] = VERIFY_ROW(KIND_NONE, 4, PIPE_CHUNK_VERIFY, PIPE_FIRST_CHUNK_VERIFY),
    [OP_VERIFY_KEYED_RLC] = VERIFY_ROW(KIND_NONE, 4, CHUNK_MAX, CHUNK_MAX),
    [OP_SIGN] = { .n_in = 2, .in_w = { 32, 32, 0 }, .out_w = 64, .has_msgs = 1, .run = run_sign, .wipe = WIPE_IN0, .chain = 1, .kind = KIND_SIGN },
    [OP_SIGN_UNMERGED] = { .n_in = 2, .in_w = { 32, 32, 0 }, .out_w = 64, .has_msgs = 1, .run = run_sign, .wipe = WIPE_IN0, .chain = 1, .kind = KIND_NONE },
    [OP_SIGN_KEYED] = { .n_in = 1, .in_w = { 4, 0, 0 }, .out_w = 64, .has_msgs = 1, .run = run_sign, .wipe = WIPE_IN0 | WIPE_OUT, .chain = 1,
                    .kind = KIND_NONE },
    [OP_X25519] = { .n_in = 2, .in_w = { 32, 32, 0 }, .out_w = 32, .run = run_x25519, .wipe = WIPE_IN0 | WIPE_OUT, .chain = 1, .kind = KIND_X25519 },
    [OP_GENPUB] = { .n_in = 1, .in_w = { 32, 0, 0 }, .out_w = 32, .run = run_genpub, .wipe = WIPE_IN0, .chain = 1, .kind = KIND_GENPUB },
    [OP_XBASE] = { .n_in = 1, .in_w = { 32, 0, 0 }, .out_w = 32, .run = run_xbase, .wipe = WIPE_IN0, .chain = 1, .kind = KIND_XBASE },
    [OP_PK_TO_X] = { .n_in = 1, .in_w = { 32, 0, 0 }, .out_w = 32, .run = run_pk_to_x, .wipe = WIPE_NONE, .chain = 1, .kind = KIND_PK_TO_X },
    [OP_SK_TO_X] = { .n_in = 1, .in_w = { 32, 0, 0 }, .out_w = 32, .run = run_sk_to_x, .wipe = WIPE_IN0 | WIPE_OUT, .chain = 1, .kind = KIND_SK_TO_X },
    [OP_CLASSIFY] = { .n_in = 1, .in_w = { 32, 0, 0 }, .out_w = 1, .run = run_classify, .wipe = WIPE_NONE, .chain = 1, .kind = KIND_NONE },
    [OP_POINT_MULADD] = { .n_in = 3, .in_w = { 32, 32, 32 }, .out_w = 32, .run = run_muladd, .wipe = WIPE_NONE, .chain = 1, .kind = KIND_NONE },
    [OP_POINT_MULADD_MUL] = { .n_in = 2, .in_w = { 32, 32, 0 }, .out_w = 32, .run = run_muladd_mul, .wipe = WIPE_NONE, .chain = 1, .kind = KIND_NONE },
    [OP_POINT_MULADD_ADD] = { .n_in = 2, .in_w = { 32, 32, 0 }, .out_w = 32, .run = run_muladd_add, .wipe = WIPE_NONE, .chain = 1, .kind = KIND_NONE },
    [OP_POINT_MULADD_POINTS] = { .n_in = 1, .in_w = { 32, 0, 0 }, .out_w = 32, .run = run_muladd_points, .wipe = WIPE_NONE, .chain = 1,
                                 .kind = KIND_NONE },
};

/* a call of operation `id` (in1, msgs, msg_off: NULL where the operation has none) */
static struct hjob job(int id, uint8_t *out, const uint8_t *in0, const uint8_t *in1, const uint8_t *msgs,
                       const uint64_t *msg_off, size_t msg_len)
{
    const struct hjob j = { .op = &g_ops[id], .in = { in0, in1, NULL }, .msgs = msgs, .msg_off = msg_off, .msg_len = msg_len, .out = out };
    return j;
}

/* ------------------------------------------------------------------------------------------
 * host-pointer entry points (include/eddsa_amd.h)
 * ---------------------------------------------------------------------------------------- */

/* The one body of the host-pointer verify and sign forms: the checks every form shares (engine.h: msg_call_open; the ctx / ph
 * prefix it builds lives on this frame for the length of the call), the row the call's form selects, the job.  A call over a
 * signer set has its WHOLE index array checked first - an index outside the set ends the call before anything is touched (the
 * device-pointer forms, which cannot look, write 64 zero bytes for such an item).  The combination's statistics go through a
 * local array, so that the caller's words change only when the call got as far as its batch size. */
static int msg_call_run(const struct msg_call *c, int sign)
{
    edk_dom dom_buf;
    uint32_t local[4] = { 0, 0, 0, 0 };
    struct hjob j = { .in = { c->first, c->second, NULL }, .out = c->out, .msgs = c->msgs, .msg_off = c->msg_off, .msg_len = c->msg_len,
                      .ks = c->ks, .sg = c->sg, .digest = c->digest, .stats = c->rlc ? local : NULL };
    int rc = msg_call_open(c, &dom_buf, &j.dom);
    if (rc < 0) return rc;
    if (rc == 0 && c->sg) {
        const uint32_t *key_idx = (const uint32_t *)c->first;
        uint32_t bad = 0;
        for (size_t i = 0; i < c->n; i++) bad |= (uint32_t)(key_idx[i] >= c->sg->count);
        if (bad) return -(int)hipErrorInvalidValue;
    }
    if (c->records) { j.stride = c->stride; j.rec_sig = c->rec_sig; j.rec_pub = c->rec_pub; j.rec_msg = c->rec_msg; }
    j.op = &g_ops[sign ? (c->sg ? OP_SIGN_KEYED : c->ctx ? OP_SIGN_UNMERGED : OP_SIGN)
                  : c->records ? OP_VERIFY_RECORDS
                  : c->ks ? (c->rlc ? OP_VERIFY_KEYED_RLC : OP_VERIFY_KEYED)
                  : c->rlc ? OP_VERIFY_RLC : c->digest || c->ctx ? OP_VERIFY_UNMERGED : OP_VERIFY];
    rc = rc ? 0 : pipe_run(j, c->n);
    if (c->stats) memcpy(c->stats, local, sizeof(local));
    return rc;
}

int ed25519_verify_batch(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs, const uint8_t *msgs,
                         const uint64_t *msg_off, size_t msg_len, size_t n)
{
    const struct msg_call c = { .out = ok, .first = sigs, .second = pubs, .msgs = msgs, .msg_off = msg_off, .msg_len = msg_len, .n = n };
    return msg_call_run(&c, 0);
}

int ed25519_verify_batch_rlc(uint8_t *ok, uint32_t stats[4], const uint8_t *sigs, const uint8_t *pubs,
                             const uint8_t *msgs, const uint64_t *msg_off, size_t msg_len, size_t n)
{
    const struct msg_call c = { .out = ok, .stats = stats, .first = sigs, .second = pubs, .msgs = msgs, .msg_off = msg_off, .msg_len = msg_len,
                                .n = n, .rlc = 1 };
    return msg_call_run(&c, 0);
}

int ed25519_verify_digests(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs, const uint8_t *digests, size_t n)
{
    const struct msg_call c = { .out = ok, .first = sigs, .second = pubs, .msgs = digests, .msg_len = EDDSA_DIGEST_BYTES, .n = n, .digest = 1 };
    return msg_call_run(&c, 0);
}

int ed25519_verify_digests_rlc(uint8_t *ok, uint32_t stats[4], const uint8_t *sigs, const uint8_t *pubs, const uint8_t *digests, size_t n)
{
    const struct msg_call c = { .out = ok, .stats = stats, .first = sigs, .second = pubs, .msgs = digests, .msg_len = EDDSA_DIGEST_BYTES, .n = n,
                                .digest = 1, .rlc = 1 };
    return msg_call_run(&c, 0);
}

int ed25519_verify_records(uint8_t *ok, const uint8_t *records, size_t stride, size_t sig_off, size_t pub_off,
                           size_t msg_off, size_t msg_len, size_t n)
{
    const struct msg_call c = { .out = ok, .first = records, .msg_len = msg_len, .n = n,
                                .records = 1, .stride = stride, .rec_sig = sig_off, .rec_pub = pub_off, .rec_msg = msg_off };
    return msg_call_run(&c, 0);
}

int ed25519ctx_verify_batch(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs, const uint8_t *msgs, const uint64_t *msg_off,
                            size_t msg_len, size_t n, const uint8_t *context, size_t context_len)
{
    const struct msg_call c = { .out = ok, .first = sigs, .second = pubs, .msgs = msgs, .msg_off = msg_off, .msg_len = msg_len, .n = n,
                                .ctx = CTX_ED25519CTX, .context = context, .context_len = context_len };
    return msg_call_run(&c, 0);
}

int ed25519ph_verify_batch(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs, const uint8_t *prehashes, size_t n,
                           const uint8_t *context, size_t context_len)
{
    const struct msg_call c = { .out = ok, .first = sigs, .second = pubs, .msgs = prehashes, .msg_len = EDDSA_PREHASH_BYTES, .n = n,
                                .ctx = CTX_ED25519PH, .context = context, .context_len = context_len };
    return msg_call_run(&c, 0);
}

/* key-set verification (include/eddsa_amd.h): 4 bytes of index per item travel where the other forms upload 32 bytes of key; the
 * key set travels in the job, and the call runs on the key set's device */
int ed25519_verify_keyed(uint8_t *ok, const eddsa_amd_keyset *ks, const uint32_t *key_idx, const uint8_t *sigs,
                         const uint8_t *msgs, const uint64_t *msg_off, size_t msg_len, size_t n)
{
    const struct msg_call c = { .out = ok, .first = sigs, .second = (const uint8_t *)key_idx, .msgs = msgs, .msg_off = msg_off, .msg_len = msg_len,
                                .n = n, .keyed = 1, .ks = ks };
    return msg_call_run(&c, 0);
}

int ed25519_verify_keyed_rlc(uint8_t *ok, uint32_t stats[4], const eddsa_amd_keyset *ks, const uint32_t *key_idx,
                             const uint8_t *sigs, const uint8_t *msgs, const uint64_t *msg_off, size_t msg_len, size_t n)
{
    const struct msg_call c = { .out = ok, .stats = stats, .first = sigs, .second = (const uint8_t *)key_idx, .msgs = msgs, .msg_off = msg_off,
                                .msg_len = msg_len, .n = n, .keyed = 1, .ks = ks, .rlc = 1 };
    return msg_call_run(&c, 0);
}

int ed25519_verify_keyed_digests(uint8_t *ok, const eddsa_amd_keyset *ks, const uint32_t *key_idx, const uint8_t *sigs,
                                 const uint8_t *digests, size_t n)
{
    const struct msg_call c = { .out = ok, .first = sigs, .second = (const uint8_t *)key_idx, .msgs = digests, .msg_len = EDDSA_DIGEST_BYTES,
                                .n = n, .keyed = 1, .ks = ks, .digest = 1 };
    return msg_call_run(&c, 0);
}

int ed25519_verify_keyed_digests_rlc(uint8_t *ok, uint32_t stats[4], const eddsa_amd_keyset *ks, const uint32_t *key_idx,
                                     const uint8_t *sigs, const uint8_t *digests, size_t n)
{
    const struct msg_call c = { .out = ok, .stats = stats, .first = sigs, .second = (const uint8_t *)key_idx, .msgs = digests,
                                .msg_len = EDDSA_DIGEST_BYTES, .n = n, .keyed = 1, .ks = ks, .digest = 1, .rlc = 1 };
    return msg_call_run(&c, 0);
}

int ed25519ctx_verify_keyed(uint8_t *ok, const eddsa_amd_keyset *ks, const uint32_t *key_idx, const uint8_t *sigs, const uint8_t *msgs,
                            const uint64_t *msg_off, size_t msg_len, size_t n, const uint8_t *context, size_t context_len)
{
    const struct msg_call c = { .out = ok, .first = sigs, .second = (const uint8_t *)key_idx, .msgs = msgs, .msg_off = msg_off, .msg_len = msg_len,
                                .n = n, .keyed = 1, .ks = ks, .ctx = CTX_ED25519CTX, .context = context, .context_len = context_len };
    return msg_call_run(&c, 0);
}

int ed25519ph_verify_keyed(uint8_t *ok, const eddsa_amd_keyset *ks, const uint32_t *key_idx, const uint8_t *sigs, const uint8_t *prehashes,
                           size_t n, const uint8_t *context, size_t context_len)
{
    const struct msg_call c = { .out = ok, .first = sigs, .second = (const uint8_t *)key_idx, .msgs = prehashes, .msg_len = EDDSA_PREHASH_BYTES,
                                .n = n, .keyed = 1, .ks = ks, .ctx = CTX_ED25519PH, .context = context, .context_len = context_len };
    return msg_call_run(&c, 0);
}

int ed25519_sign_batch(uint8_t *sigs, const uint8_t *secs, const uint8_t *pubs, const uint8_t *msgs,
                       const uint64_t *msg_off, size_t msg_len, size_t n)
{
    const struct msg_call c = { .out = sigs, .first = secs, .second = pubs, .msgs = msgs, .msg_off = msg_off, .msg_len = msg_len, .n = n };
    return msg_call_run(&c, 1);
}

int ed25519ctx_sign_batch(uint8_t *sigs, const uint8_t *secs, const uint8_t *pubs, const uint8_t *msgs, const uint64_t *msg_off,
                          size_t msg_len, size_t n, const uint8_t *context, size_t context_len)
{
    const struct msg_call c = { .out = sigs, .first = secs, .second = pubs, .msgs = msgs, .msg_off = msg_off, .msg_len = msg_len, .n = n,
                                .ctx = CTX_ED25519CTX, .context = context, .context_len = context_len };
    return msg_call_run(&c, 1);
}

int ed25519ph_sign_batch(uint8_t *sigs, const uint8_t *secs, const uint8_t *pubs, const uint8_t *prehashes, size_t n,
                         const uint8_t *context, size_t context_len)
{
    const struct msg_call c = { .out = sigs, .first = secs, .second = pubs, .msgs = prehashes, .msg_len = EDDSA_PREHASH_BYTES, .n = n,
                                .ctx = CTX_ED25519PH, .context = context, .context_len = context_len };
    return msg_call_run(&c, 1);
}

/* signing over a signer set (include/eddsa_amd.h) */
int ed25519_sign_keyed(uint8_t *sigs, const eddsa_amd_signer *s, const uint32_t *key_idx, const uint8_t *msgs, const uint64_t *msg_off,
                       size_t msg_len, size_t n)
{
    const struct msg_call c = { .out = sigs, .first = (const uint8_t *)key_idx, .msgs = msgs, .msg_off = msg_off, .msg_len = msg_len, .n = n,
                                .keyed = 1, .sg = s };
    return msg_call_run(&c, 1);
}

int ed25519ctx_sign_keyed(uint8_t *sigs, const eddsa_amd_signer *s, const uint32_t *key_idx, const uint8_t *msgs, const uint64_t *msg_off,
                          size_t msg_len, size_t n, const uint8_t *context, size_t context_len)
{
    const struct msg_call c = { .out = sigs, .first = (const uint8_t *)key_idx, .msgs = msgs, .msg_off = msg_off, .msg_len = msg_len, .n = n,
                                .keyed = 1, .sg = s, .ctx = CTX_ED25519CTX, .context = context, .context_len = context_len };
    return msg_call_run(&c, 1);
}

int ed25519ph_sign_keyed(uint8_t *sigs, const eddsa_amd_signer *s, const uint32_t *key_idx, const uint8_t *prehashes, size_t n,
                         const uint8_t *context, size_t context_len)
{
    const struct msg_call c = { .out = sigs, .first = (const uint8_t *)key_idx, .msgs = prehashes, .msg_len = EDDSA_PREHASH_BYTES, .n = n,
                                .keyed = 1, .sg = s, .ctx = CTX_ED25519PH, .context = context, .context_len = context_len };
    return msg_call_run(&c, 1);
}

int x25519_batch(uint8_t *out, const uint8_t *scalars, const uint8_t *points, size_t n) { return pipe_run(job(OP_X25519, out, scalars, points, NULL, NULL, 0), n); }

int ed25519_genpub_batch(uint8_t *pubs, const uint8_t *secs, size_t n) { return pipe_run(job(OP_GENPUB, pubs, secs, NULL, NULL, NULL, 0), n); }
int x25519_base_batch(uint8_t *out, const uint8_t *scalars, size_t n) { return pipe_run(job(OP_XBASE, out, scalars, NULL, NULL, NULL, 0), n); }
int pk_ed25519_to_x25519_batch(uint8_t *out, const uint8_t *in, size_t n) { return pipe_run(job(OP_PK_TO_X, out, in, NULL, NULL, NULL, 0), n); }
int sk_ed25519_to_x25519_batch(uint8_t *out, const uint8_t *in, size_t n) { return pipe_run(job(OP_SK_TO_X, out, in, NULL, NULL, NULL, 0), n); }

/* point classification (include/eddsa_amd.h): an empty batch is done and NULLs are refused before any device is asked */
int ed25519_point_classify_batch(uint8_t *cls, const uint8_t *points, size_t n)
{
    if (n == 0) return 0;
    if (!cls || !points) return -(int)hipErrorInvalidValue;
    return pipe_run(job(OP_CLASSIFY, cls, points, NULL, NULL, NULL, 0), n);
}

/* [m]P + [a]B (include/eddsa_amd.h): an empty batch is done and NULLs are refused before any device is asked; the row is chosen by
 * which scalar arrays the caller gave */
int ed25519_point_muladd_batch(uint8_t *out, const uint8_t *points, const uint8_t *mul, const uint8_t *add, size_t n)
{
    if (n == 0) return 0;
    if (!out || !points) return -(int)hipErrorInvalidValue;
    const struct hjob j = { .op = &g_ops[mul && add ? OP_POINT_MULADD : mul ? OP_POINT_MULADD_MUL : add ? OP_POINT_MULADD_ADD : OP_POINT_MULADD_POINTS],
                            .in = { points, mul ? mul : add, mul ? add : NULL }, .out = out };
    return pipe_run(j, n);
}

/* ------------------------------------------------------------------------------------------
 * several devices in one process, host-pointer forms: thread d runs the ordinary pipeline of device d
 * on shard d; results are copied device -> caller's buffer slice directly, so there is nothing to gather
 * ---------------------------------------------------------------------------------------- */

struct shard_job { struct hjob j; size_t n; int device; int rc; };

static void *shard_thread(void *arg)
{
    struct shard_job *s = (struct shard_job *)arg;
    struct call c;
    s->rc = enter(&c, s->device);
    if (s->rc) return NULL;
    s->rc = pipe_run_on(c.e, &s->j, s->n, 0);
    leave(&c);
    return NULL;
}

/* split job j over the device set: item ranges for the fixed-width arrays, message bytes for ragged ones */
static int multi_run(const struct hjob whole, size_t n)
{
    const struct hjob *j = &whole;
    struct shard_job jobs[MAX_DEVICES];
    pthread_t th[MAX_DEVICES];
    uint64_t *offs[MAX_DEVICES] = { NULL };
    int started[MAX_DEVICES] = { 0 };
    int rc = 0, g;
    pthread_rwlock_rdlock(&g_table);
    g = g_multi.n;
    for (int d = 0; d < g; d++) jobs[d].device = g_multi.dev[d];
    pthread_rwlock_unlock(&g_table);
    if (g == 0) return -(int)hipErrorNotInitialized;
    if (n == 0) return 0;
    for (int d = 0; d < g; d++) {
        size_t lo, hi;
        eddsa_amd_shard_bounds(n, d, g, &lo, &hi);
        jobs[d].j = *j;
        jobs[d].n = hi - lo;
        jobs[d].rc = 0;
        for (int i = 0; i < j->op->n_in; i++) jobs[d].j.in[i] = j->in[i] + lo * in_w(j, i);
        jobs[d].j.out = j->out + lo * j->op->out_w;
        if (j->op->has_msgs && j->msg_off) {        /* ragged: the shard's own offset table, rebased to 0 */
            offs[d] = (uint64_t *)malloc((hi - lo + 1) * sizeof(uint64_t));
            if (!offs[d]) { rc = -(int)hipErrorOutOfMemory; break; }
            offsets_rebase(offs[d], j->msg_off + lo, hi - lo);
            jobs[d].j.msg_off = offs[d];
            jobs[d].j.msgs = j->msgs + j->msg_off[lo];
        } else if (j->op->has_msgs) {
            jobs[d].j.msgs = j->msgs + lo * j->msg_len;
        }
    }
    for (int d = 0; d < g && !rc; d++) {
        if (jobs[d].n == 0) continue;
        if (pthread_create(&th[d], NULL, shard_thread, &jobs[d]) != 0) { rc = -(int)hipErrorOutOfMemory; break; }
        started[d] = 1;
    }
    for (int d = 0; d < g; d++) {
        if (started[d]) { pthread_join(th[d], NULL); if (!rc) rc = jobs[d].rc; }
        free(offs[d]);
    }
    return rc;
}

int ed25519_verify_batch_multi(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs, const uint8_t *msgs,
                               const uint64_t *msg_off, size_t msg_len, size_t n)
{
    return multi_run(job(OP_VERIFY, ok, sigs, pubs, msgs, msg_off, msg_len), n);
}

int ed25519_verify_digests_multi(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs, const uint8_t *digests, size_t n)
{
    struct hjob j = job(OP_VERIFY_UNMERGED, ok, sigs, pubs, digests, NULL, EDDSA_DIGEST_BYTES);
    j.digest = 1;
    return multi_run(j, n);
}

int ed25519_sign_batch_multi(uint8_t *sigs, const uint8_t *secs, const uint8_t *pubs, const uint8_t *msgs,
                             const uint64_t *msg_off, size_t msg_len, size_t n)
{
    return multi_run(job(OP_SIGN, sigs, secs, pubs, msgs, msg_off, msg_len), n);
}

int x25519_batch_multi(uint8_t *out, const uint8_t *scalars, const uint8_t *points, size_t n) { return multi_run(job(OP_X25519, out, scalars, points, NULL, NULL, 0), n); }

/* ------------------------------------------------------------------------------------------
 * the eddsa.h surface: batches of one.  No error channel in these signatures, so fail loudly.
 * ---------------------------------------------------------------------------------------- */

static void must(int rc, const char *what)
{
    if (rc == 0) return;
    fprintf(stderr, "libeddsa_amd: %s failed on the GPU path: %s (no CPU fallback exists)\n", what,
            eddsa_amd_strerror(rc));
    abort();
}

void ed25519_genpub(uint8_t pub[32], const uint8_t sec[32]) { must(ed25519_genpub_batch(pub, sec, 1), "ed25519_genpub"); }
void ed25519_sign(uint8_t sig[64], const uint8_t sec[32], const uint8_t pub[32], const uint8_t *data, size_t len)
{
    must(ed25519_sign_batch(sig, sec, pub, data, NULL, len, 1), "ed25519_sign");
}
bool ed25519_verify(const uint8_t sig[64], const uint8_t pub[32], const uint8_t *data, size_t len)
{
    uint8_t ok = 0;
    must(ed25519_verify_batch(&ok, sig, pub, data, NULL, len, 1), "ed25519_verify");
    return ok != 0;
}
void x25519_base(uint8_t out[32], const uint8_t scalar[32]) { must(x25519_base_batch(out, scalar, 1), "x25519_base"); }
void x25519(uint8_t out[32], const uint8_t scalar[32], const uint8_t point[32]) { must(x25519_batch(out, scalar, point, 1), "x25519"); }
void pk_ed25519_to_x25519(uint8_t out[32], const uint8_t in[32]) { must(pk_ed25519_to_x25519_batch(out, in, 1), "pk_ed25519_to_x25519"); }
void sk_ed25519_to_x25519(uint8_t out[32], const uint8_t in[32]) { must(sk_ed25519_to_x25519_batch(out, in, 1), "sk_ed25519_to_x25519"); }

/* reference lib/ed25519-sha512.c:270-324 and lib/x25519.c:232-243: the obsolete names */
void eddsa_genpub(uint8_t pub[32], const uint8_t sec[32]) { ed25519_genpub(pub, sec); }
void eddsa_sign(uint8_t sig[64], const uint8_t sec[32], const uint8_t pub[32], const uint8_t *data, size_t len)
{
    ed25519_sign(sig, sec, pub, data, len);
}
bool eddsa_verify(const uint8_t sig[64], const uint8_t pub[32], const uint8_t *data, size_t len)
{
    return ed25519_verify(sig, pub, data, len);
}
void DH(uint8_t out[32], const uint8_t sec[32], const uint8_t point[32]) { x25519(out, sec, point); }
void eddsa_pk_eddsa_to_dh(uint8_t out[32], const uint8_t in[32]) { pk_ed25519_to_x25519(out, in); }
void eddsa_sk_eddsa_to_dh(uint8_t out[32], const uint8_t in[32]) { sk_ed25519_to_x25519(out, in); }

/* ------------------------------------------------------------------------------------------
 * measurement aids and test hooks (include/eddsa_amd_debug.h): only libeddsa_amd_debug.so has them
 * ---------------------------------------------------------------------------------------- */
#ifdef EDDSA_AMD_DEBUG_BUILD
void eddsa_amd_set_pipeline_chain(int mode)
{
    pthread_rwlock_wrlock(&g_table);
    g_pipe_chain = mode;
    pthread_rwlock_unlock(&g_table);
}

/* tuning: items of the first chunk of a host-pointer call and of its later stages (0 = default).  A measurement aid. */
void eddsa_amd_set_pipeline(size_t first_chunk, size_t stage_chunk)
{
    pthread_rwlock_wrlock(&g_table);
    g_pipe_first = first_chunk;
    g_pipe_stage = stage_chunk;
    pthread_rwlock_unlock(&g_table);
}

/* on != 0: record host-side time stamps in every host-pointer call from now on; returns the number of stamps of the last
 * call and copies up to `max` of them: tag (0 call start, 1 lane drained, 2 inputs staged and queued, 3 kernels queued,
 * 4 download queued, 5 all lanes drained, 6 call end; of a combined launch also 7 leader elected, 8 callers gathered,
 * 9 requests packed, 10 results handed back), chunk index, milliseconds since the call started.  on = 2: recording stops
 * by itself after the 20th combined launch of 32 calls or more, so that a typical launch under load can be read */
int eddsa_amd_debug_pipe_trace(int on, int *tags, unsigned *chunks, double *ms, int max)
{
    pthread_rwlock_wrlock(&g_table);       /* no call in flight: nobody is stamping */
    int n = __atomic_load_n(&g_trace.n, __ATOMIC_RELAXED);
    n = n > TRACE_MAX ? TRACE_MAX : n;
    n = n < max ? n : max;
    for (int i = 0; i < n; i++) {
        tags[i] = __atomic_load_n(&g_trace.tag[i], __ATOMIC_RELAXED); chunks[i] = __atomic_load_n(&g_trace.chunk[i], __ATOMIC_RELAXED);
        ms[i] = 1e-6 * (double)(__atomic_load_n(&g_trace.t_ns[i], __ATOMIC_RELAXED) - __atomic_load_n(&g_trace.t_ns[0], __ATOMIC_RELAXED));
    }
    __atomic_store_n(&g_trace.on, on, __ATOMIC_RELAXED);
    __atomic_store_n(&g_trace.seen, 0, __ATOMIC_RELAXED);
    pthread_rwlock_unlock(&g_table);
    return n;
}

/* test hook (inert unless armed): the next host-pointer call fails (hipErrorUnknown) after its inputs were staged and its
 * kernels launched, so that the error path's clean-up (the staging copies of secrets are wiped there too) can be exercised */
int eddsa_amd_debug_fail_next_host_call(void)
{
    if (!__atomic_load_n(&g_hooks_armed, __ATOMIC_ACQUIRE)) return EDDSA_AMD_HOOKS_OFF;
    __atomic_store_n(&g_fail_next_host_call, 1, __ATOMIC_RELEASE);
    return 0;
}

/* diagnostic: combined launches and the items they carried on the default device since its engine was built */
int eddsa_amd_combiner_stats(uint64_t out[2])
{
    struct call c;
    int rc = enter(&c, -1);
    if (rc) return rc;
    pthread_mutex_lock(&c.e->comb_q.lk);
    out[0] = c.e->comb_q.batches; out[1] = c.e->comb_q.items;
    pthread_mutex_unlock(&c.e->comb_q.lk);
    leave(&c);
    return 0;
}
#endif /* the debug build */
