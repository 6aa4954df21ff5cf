/*
 * eddsa_amd.c - engines and the device-pointer side of libeddsa_amd.so, plain C.
 *
 * One `struct engine` per HIP device (generated tables, a pool of workspaces, the host pipeline's lanes and the
 * combiner's queue, both driven by host_pipe.c), created on first use.  A device-pointer call runs on the device its
 * output buffer lives on; a host-pointer call (host_pipe.c) on the default device (eddsa_amd_init) or, for the
 * *_multi entry points, on every device of the set bound by eddsa_amd_init_devices.  Every call makes its device
 * current for its own duration and restores the caller's.
 *
 * Everything is computed by the HIP kernels in kernels.hip / rlc.hip; there is no CPU arithmetic on this side and no
 * fallback: without a usable gfx950 device every entry point fails (batch API: negative return; eddsa.h API, which has
 * no error channel: message on stderr + abort()).  Shared declarations and the lock order: engine.h.
 */
#include "engine.h"

#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

pthread_rwlock_t g_table = PTHREAD_RWLOCK_INITIALIZER;
struct engine *g_eng[MAX_DEVICES];
static int g_default = -1;            /* device of the host-pointer entry points; -1: the caller's current device at first use */
static int g_verify_algo = 0;         /* eddsa_amd_set_verify_algo: 0 by pass size (default), 1 full-length windows, 2 half-length scalars */
static int g_offcurve_mode = 1;       /* eddsa_amd_set_offcurve_mode: 0 reject, 1 exact (default), 2 all exact */
static int g_verify_policy;           /* the EDDSA_AMD_VERIFY_* bits of the same word (default 0: the reference's verdicts) */
static int g_verify_equation;         /* eddsa_amd_set_verify_equation: EDDSA_AMD_EQUATION_COFACTORLESS (default) or _COFACTORED */
static int g_profiling;               /* record marks around the three verify kernels */
static size_t g_rlc_min_items = EDDSA_AMD_RLC_MIN_ITEMS_DEFAULT;   /* eddsa_amd_set_rlc_min_items: smaller calls go to the per-item kernels */

int g_hooks_armed;                     /* eddsa_amd_debug_init: read and written atomically */
struct multi g_multi;                  /* the device set of the *_multi entry points (eddsa_amd_init_devices) */
static pthread_mutex_t g_rccl_lk = PTHREAD_MUTEX_INITIALIZER;   /* one grouped RCCL call at a time (taken after g_table) */
#define NCCL_UINT8 1                   /* ncclUint8, rccl.h */

const char *eddsa_amd_strerror(int err)
{
    if (err == 0) return "success";
    if (err == ERR_NOT_GFX950) return "eddsa_amd: device is not gfx950 (MI355X); no code object for it";
    if (err == ERR_RCCL_MISSING) return "eddsa_amd: librccl.so.1 could not be loaded (needed for the multi-device result gather)";
    if (err == EDDSA_AMD_HOOKS_OFF) return "eddsa_amd: test hooks not armed (eddsa_amd_debug_init)";
    if (err == EDDSA_AMD_STALLED) return "eddsa_amd: a verify kernel gave up waiting for a hand-off between its waves; the pass's outputs are incomplete";
    if (err <= ERR_RCCL_BASE) {
        if (g_multi.GetErrorString) return g_multi.GetErrorString(ERR_RCCL_BASE - err);
        return "eddsa_amd: RCCL error";
    }
    return hipGetErrorString((hipError_t)(-err));
}

static struct { int count, first; char what[96]; } g_teardown;   /* hip_note: count and first are atomic; what is written by the first */

void hip_note(hipError_t e, const char *what)
{
    if (e == hipSuccess) return;
    if (__atomic_fetch_add(&g_teardown.count, 1, __ATOMIC_ACQ_REL) == 0) {
        __atomic_store_n(&g_teardown.first, (int)e, __ATOMIC_RELEASE);
        strncpy(g_teardown.what, what, sizeof(g_teardown.what) - 1);
    }
    (void)hipGetLastError();               /* noted: the sticky slot is cleared (the only unchecked HIP calls of the host side are this one and hip_forget_error's) */
}

void hip_forget_error(void)
{
    (void)hipGetLastError();               /* the caller has handled the answer it stands for */
}

/* ------------------------------------------------------------------------------------------
 * engines
 * ---------------------------------------------------------------------------------------- */

/* device buffers that held secrets (or may have) are zeroed before they go back to the allocator:
 * the reference wipes after its secret-key operations (lib/ed25519-sha512.c:77,136, lib/x25519.c:208,221) */
void wipe_free(void *p, size_t bytes)
{
    if (!p) return;
    if (bytes) { HIP_NOTE(hipMemset(p, 0, bytes)); HIP_NOTE(hipDeviceSynchronize()); }
    HIP_NOTE(hipFree(p));
}

static void ws_release(struct vslot *v)
{
    if (v->ws.digits) HIP_NOTE(hipFree(v->ws.digits));
    if (v->ws.table) HIP_NOTE(hipFree(v->ws.table));
    if (v->ws.acc) HIP_NOTE(hipFree(v->ws.acc));
    if (v->ws.flags) HIP_NOTE(hipFree(v->ws.flags));
    if (v->ws.hdigits) HIP_NOTE(hipFree(v->ws.hdigits));
    if (v->ws.rtable) HIP_NOTE(hipFree(v->ws.rtable));
    if (v->ws.offlist) HIP_NOTE(hipFree(v->ws.offlist));
    if (v->ws.onlist) HIP_NOTE(hipFree(v->ws.onlist));
    if (v->ws.perm) HIP_NOTE(hipFree(v->ws.perm));
    if (v->ws.lenbins) HIP_NOTE(hipFree(v->ws.lenbins));
    if (v->ws.offcount) HIP_NOTE(hipFree(v->ws.offcount));
    if (v->ws.exact_pad) HIP_NOTE(hipFree(v->ws.exact_pad));
    if (v->ws.sums) HIP_NOTE(hipFree(v->ws.sums));
    if (v->ws.domdig) HIP_NOTE(hipFree(v->ws.domdig));
    if (v->ws.keybytes) HIP_NOTE(hipFree(v->ws.keybytes));
    if (v->ws.gsigs) HIP_NOTE(hipFree(v->ws.gsigs));
    v->ws.capacity = 0;
    v->ws.digits = v->ws.table = v->ws.acc = v->ws.offlist = v->ws.offcount = v->ws.exact_pad = NULL;
    v->ws.hdigits = v->ws.rtable = v->ws.sums = v->ws.onlist = v->ws.perm = v->ws.lenbins = NULL;
    v->ws.flags = NULL;
    v->ws.domdig = NULL;
    v->ws.keybytes = NULL;
    v->ws.gsigs = NULL;
}

/* bytes of the two secret-bearing buffers of a fixed-base workspace of `cap` items */
static size_t fws_acc_bytes(size_t cap) { return cap * ACC_WORDS * sizeof(uint32_t); }
static size_t fws_aux_bytes(size_t cap) { return cap * 16 * sizeof(uint32_t); }

static void fws_release(struct vslot *v)
{
    wipe_free(v->fws.acc, fws_acc_bytes(v->fws.capacity));
    wipe_free(v->fws.aux, fws_aux_bytes(v->fws.capacity));
    if (v->fws.tiles) HIP_NOTE(hipFree(v->fws.tiles));
    if (v->fws.perm) HIP_NOTE(hipFree(v->fws.perm));
    if (v->fws.lenbins) HIP_NOTE(hipFree(v->fws.lenbins));
    memset(&v->fws, 0, sizeof(v->fws));
}

static void rws_release(struct vslot *v)
{
    if (v->rws.base) HIP_NOTE(hipFree(v->rws.base));
    if (v->rws.host_gok) HIP_NOTE(hipHostFree(v->rws.host_gok));
    memset(&v->rws, 0, sizeof(v->rws));
}

static size_t round_capacity(size_t items)
{
    size_t cap = (items + VERIFY_TILE - 1) / VERIFY_TILE * VERIFY_TILE;
    return (cap + 8 * VERIFY_TILE - 1) / (8 * VERIFY_TILE) * (8 * VERIFY_TILE);   /* whole finish blocks */
}

/* caller holds e->lk; st = the stream the pass is about to use */
static int fws_reserve(struct vslot *v, size_t items, hipStream_t st)
{
    int rc = 0;
    const size_t cap = round_capacity(items);
    if (cap <= v->fws.capacity) return 0;
    TRY(hipEventSynchronize(v->free));
    fws_release(v);
    TRY(hipMalloc((void **)&v->fws.acc, fws_acc_bytes(cap)));
    TRY(hipMalloc((void **)&v->fws.aux, fws_aux_bytes(cap)));
    /* recycled memory: start clean.  On the pass's own stream: a hipMemset on the null stream is not ordered
     * with the kernels of a non-blocking stream and could land after their first stores */
    TRY(hipMemsetAsync(v->fws.acc, 0, fws_acc_bytes(cap), st));
    TRY(hipMemsetAsync(v->fws.aux, 0, fws_aux_bytes(cap), st));
    TRY(hipMalloc((void **)&v->fws.perm, cap * sizeof(uint32_t)));
    TRY(hipMalloc((void **)&v->fws.lenbins, 2 * EDK_LEN_BINS * sizeof(uint32_t)));
    TRY(hipMalloc((void **)&v->fws.tiles, EDK_TILES_BYTES));
    TRY(hipMemsetAsync(v->fws.tiles, 0, EDK_TILES_BYTES, st));
    v->fws.capacity = cap;
out:
    if (rc) fws_release(v);
    return rc;
}

/* caller holds e->lk */
static int ws_reserve(struct vslot *v, size_t items)
{
    int rc = 0;
    const size_t cap = round_capacity(items);
    if (cap <= v->ws.capacity) return 0;
    /* the old buffers may still be in use by enqueued kernels */
    TRY(hipEventSynchronize(v->free));
    ws_release(v);
    TRY(hipMalloc((void **)&v->ws.digits, cap * VERIFY_DIGIT_WORDS * sizeof(uint32_t)));
    TRY(hipMalloc((void **)&v->ws.table, cap / VERIFY_TILE * (size_t)VERIFY_TABLE_WORDS_PER_TILE * sizeof(uint32_t)));
    TRY(hipMalloc((void **)&v->ws.acc, cap * ACC_WORDS * sizeof(uint32_t)));
    TRY(hipMalloc((void **)&v->ws.hdigits, cap * HALF_DIGIT_WORDS * sizeof(uint32_t)));
    TRY(hipMalloc((void **)&v->ws.rtable, cap / VERIFY_TILE * (size_t)VERIFY_TABLE_WORDS_PER_TILE * sizeof(uint32_t)));
    TRY(hipMalloc((void **)&v->ws.flags, cap));
    TRY(hipMalloc((void **)&v->ws.offlist, cap * sizeof(uint32_t)));
    TRY(hipMalloc((void **)&v->ws.onlist, cap * sizeof(uint32_t)));
    TRY(hipMalloc((void **)&v->ws.perm, cap * sizeof(uint32_t)));
    TRY(hipMalloc((void **)&v->ws.lenbins, 2 * EDK_LEN_BINS * sizeof(uint32_t)));
    TRY(hipMalloc((void **)&v->ws.offcount, EDK_OFFCOUNT_BYTES));
    TRY(hipMemset(v->ws.offcount, 0, EDK_OFFCOUNT_BYTES));
    TRY(hipStreamSynchronize(NULL));      /* the pass's stream does not wait for the null stream */
    TRY(hipMalloc((void **)&v->ws.exact_pad, EDK_EXACT_PAD_BYTES));
    TRY(hipMalloc((void **)&v->ws.sums, EDK_SUMS_BYTES));
    TRY(hipMalloc((void **)&v->ws.domdig, cap * EDK_DOM_DIGEST_BYTES));
    TRY(hipMalloc((void **)&v->ws.keybytes, cap * 32));   /* keyed passes: the items' key bytes */
    v->ws.capacity = cap;
out:
    if (rc) ws_release(v);
    return rc;
}

/* caller holds e->lk */
static int rws_reserve(struct vslot *v, size_t items)
{
    int rc = 0;
    const size_t cap = round_capacity(items);
    if (cap <= v->rws.capacity) return 0;
    TRY(hipEventSynchronize(v->free));
    rws_release(v);
    TRY(hipMalloc((void **)&v->rws.base, edk_rlc_ws_bytes(cap)));
    TRY(hipMemset((char *)v->rws.base + edk_rlc_hook_offset(cap), 0, 256));
    TRY(hipStreamSynchronize(NULL));      /* the pass's stream does not wait for the null stream */
    TRY(hipHostMalloc(&v->rws.host_gok, EDK_RLC_HOST_BYTES, hipHostMallocDefault));
    v->rws.capacity = cap;
out:
    if (rc) rws_release(v);
    return rc;
}

/* caller holds e->lk: the slot a pass on stream `st` uses.  Slots marked busy (rlc_on, while it waits for its
 * stream outside the lock) are not handed out; when all are, the caller waits for one to be released. */
static struct vslot *ws_pick(struct engine *e, hipStream_t st)
{
    for (;;) {
        struct vslot *idle = NULL, *lru = NULL;
        for (int i = 0; i < VERIFY_SLOTS; i++) {
            struct vslot *v = &e->vs[i];
            if (v->busy) continue;
            if (v->stamp && v->last_stream == st) { lru = v; idle = NULL; break; }
            if (!idle && (v->stamp == 0 || hipEventQuery(v->free) == hipSuccess)) idle = v;
            if (!lru || v->stamp < lru->stamp) lru = v;
        }
        if (idle) lru = idle;
        if (lru) {
            lru->last_stream = st;
            lru->stamp = ++e->clock;
            return lru;
        }
        pthread_cond_wait(&e->slot_cv, &e->lk);
    }
}

/* everything an engine holds on its device.  Caller holds g_table for writing (no call is in
 * flight) and has made e->device current. */
static void engine_destroy(struct engine *e)
{
    HIP_NOTE(hipDeviceSynchronize());
    pipe_release(&e->pipe);
    combiner_release(&e->comb_q);
    for (int i = 0; i < VERIFY_SLOTS; i++) {
        struct vslot *v = &e->vs[i];
        ws_release(v);
        fws_release(v);
        rws_release(v);
        if (v->ws.side) HIP_NOTE(hipStreamDestroy(v->ws.side));
        if (v->ws.ev_prepared) HIP_NOTE(hipEventDestroy(v->ws.ev_prepared));
        if (v->ws.ev_exact) HIP_NOTE(hipEventDestroy(v->ws.ev_exact));
        if (v->free) HIP_NOTE(hipEventDestroy(v->free));
    }
    if (e->base16) HIP_NOTE(hipFree(e->base16));
    if (e->comb) HIP_NOTE(hipFree(e->comb));
    if (e->comb_img) HIP_NOTE(hipFree(e->comb_img));
    if (e->status) HIP_NOTE(hipHostFree(e->status));
    for (int s = 0; s < MARK_SLOTS; s++)
        for (int i = 0; i < 4; i++) if (e->marks[s][i]) HIP_NOTE(hipEventDestroy(e->marks[s][i]));
    pthread_mutex_destroy(&e->lk);
    pthread_mutex_destroy(&e->pipe_lk);
    pthread_cond_destroy(&e->slot_cv);
    free(e);
}

/* caller holds g_table for writing */
static int engine_create(int device)
{
    int rc = 0, saved = -1;
    hipDeviceProp_t prop;
    struct engine *e;
    if (device < 0 || device >= MAX_DEVICES) return -(int)hipErrorInvalidDevice;
    if (g_eng[device]) return 0;
    e = (struct engine *)calloc(1, sizeof(*e));
    if (!e) return -(int)hipErrorOutOfMemory;
    e->device = device;
    pthread_mutex_init(&e->lk, NULL);
    pthread_mutex_init(&e->pipe_lk, NULL);
    pthread_cond_init(&e->slot_cv, NULL);
    combiner_init(&e->comb_q);
    pipe_setup(&e->pipe);
    HIP_NOTE(hipGetDevice(&saved));
    TRY(hipSetDevice(device));
    TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) { rc = ERR_NOT_GFX950; goto out; }
    TRY(hipMalloc((void **)&e->base16, (size_t)2 * TABLE_BASE16_ENTRIES * TABLE_ENTRY_WORDS * sizeof(uint32_t)));
    TRY(hipMalloc((void **)&e->comb, TABLE_COMB_ENTRIES * TABLE_ENTRY_WORDS * sizeof(uint32_t)));
    TRY(hipMalloc((void **)&e->comb_img, COMB_IMG_WORDS * sizeof(uint32_t)));
    TRY(hipHostMalloc((void **)&e->status, 64, hipHostMallocDefault));
    memset(e->status, 0, 64);
    for (int i = 0; i < VERIFY_SLOTS; i++) {
        /* highest queue priority for the side streams: their few workgroups must be dispatched while
         * k_verify_main still has thousands waiting, not after them */
        int lo = 0, hi = 0;
        struct vslot *v = &e->vs[i];
        v->ws.status = e->status;
        TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
        TRY(hipStreamCreateWithPriority(&v->ws.side, hipStreamNonBlocking, hi));
        TRY(hipEventCreateWithFlags(&v->ws.ev_prepared, hipEventDisableTiming));
        TRY(hipEventCreateWithFlags(&v->ws.ev_exact, hipEventDisableTiming));
        TRY(hipEventCreateWithFlags(&v->free, hipEventDisableTiming));
        TRY(hipEventRecord(v->free, NULL));
    }
    for (int s = 0; s < MARK_SLOTS; s++)
        for (int i = 0; i < 4; i++) TRY(hipEventCreate(&e->marks[s][i]));
    TRY(edk_init_tables(e->base16, e->comb, e->comb_img, NULL));
    TRY(hipDeviceSynchronize());
    g_eng[device] = e;
    e = NULL;
out:
    if (e) engine_destroy(e);          /* a half-built engine leaks nothing */
    if (saved >= 0) HIP_NOTE(hipSetDevice(saved));
    return rc;
}

/* Every call brackets its work with enter()/leave(): enter() resolves the engine (creating it on
 * first use), holds g_table for reading and makes the engine's device current for the calling
 * thread; leave() restores the caller's device.  device < 0: the default device. */
int enter(struct call *c, int device)
{
    c->e = NULL;
    c->saved = -1;
    /* (an engine built here can be torn down again by a concurrent eddsa_amd_shutdown before this thread holds the table
     * for reading: then it is built once more; only a storm of shutdowns could use up the attempts) */
    for (int attempt = 0; attempt < 16; attempt++) {
        pthread_rwlock_rdlock(&g_table);
        int dev = device >= 0 ? device : g_default;
        if (dev < 0) {                     /* never bound: the caller's current device becomes the default */
            hipError_t er = hipGetDevice(&dev);
            if (er != hipSuccess) { pthread_rwlock_unlock(&g_table); return -(int)er; }
        }
        if (dev >= MAX_DEVICES) { pthread_rwlock_unlock(&g_table); return -(int)hipErrorInvalidDevice; }
        if (g_eng[dev]) {
            hipError_t er;
            c->e = g_eng[dev];
            HIP_NOTE(hipGetDevice(&c->saved));
            er = hipSetDevice(dev);
            if (er != hipSuccess) { pthread_rwlock_unlock(&g_table); return -(int)er; }
            return 0;
        }
        pthread_rwlock_unlock(&g_table);
        pthread_rwlock_wrlock(&g_table);
        int rc = engine_create(dev);
        if (rc == 0 && device < 0 && g_default < 0) g_default = dev;
        pthread_rwlock_unlock(&g_table);
        if (rc) return rc;
    }
    return -(int)hipErrorNotReady;         /* shut down again between the two steps */
}

void leave(struct call *c)
{
    if (c->saved >= 0) HIP_NOTE(hipSetDevice(c->saved));
    pthread_rwlock_unlock(&g_table);
}

/* the device a device-pointer call runs on: where its output buffer lives */
static int device_of(const void *p, int *device)
{
    hipPointerAttribute_t a;
    hipError_t er = hipPointerGetAttributes(&a, p);
    if (er != hipSuccess) { hip_forget_error(); return -(int)hipErrorInvalidValue; }
    if (a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged) return -(int)hipErrorInvalidValue;
    *device = a.device;
    return 0;
}

int eddsa_amd_init(int device)
{
    struct call c;
    int rc;
    if (device < 0) return -(int)hipErrorInvalidDevice;
    rc = enter(&c, device);
    if (rc) return rc;
    leave(&c);
    pthread_rwlock_wrlock(&g_table);
    g_default = device;
    pthread_rwlock_unlock(&g_table);
    return 0;
}

static void multi_release(void)
{
    for (int i = 0; i < g_multi.n; i++)
        if (g_multi.comm[i] && g_multi.CommDestroy) (void)g_multi.CommDestroy(g_multi.comm[i]);
    void *h = g_multi.rccl;
    memset(&g_multi, 0, sizeof(g_multi));
    g_multi.rccl = h;                  /* the library stays loaded; its symbols are looked up again */
}

void eddsa_amd_shutdown(void)
{
    int saved = -1;
    pthread_rwlock_wrlock(&g_table);
    HIP_NOTE(hipGetDevice(&saved));
    multi_release();
    for (int d = 0; d < MAX_DEVICES; d++) {
        if (!g_eng[d]) continue;
        HIP_NOTE(hipSetDevice(d));
        engine_destroy(g_eng[d]);
        g_eng[d] = NULL;
    }
    g_default = -1;
    __atomic_store_n(&g_hooks_armed, 0, __ATOMIC_RELEASE);
    edk_debug_counting(0);
    (void)edk_debug_fail_in(0);
    if (saved >= 0) HIP_NOTE(hipSetDevice(saved));   /* teardown: nothing to report to */
    pthread_rwlock_unlock(&g_table);
    host_pool_stop();
}

/* ------------------------------------------------------------------------------------------
 * settings
 * ---------------------------------------------------------------------------------------- */

/* How verify treats a public key that does not decode to a curve point (ed_import never fails,
 * reference lib/ed.c:100-149).  EXACT (default): such items are evaluated in the reference's own
 * order of operations, which is the only way to reproduce its bytes there.  REJECT: they are
 * rejected outright; this differs from the reference only if encode(C) == R for a C that depends on
 * SHA-512(R || A || M), i.e. on a fixed point of a random function, and saves the ~1 ms the exact
 * pass costs whenever a batch contains such keys.  ALL (2): every item takes the reference-order
 * path and the windowed evaluation's result is ignored -- slow (latency-bound), for self-checks.
 * Bits 8-11 of the word (EDDSA_AMD_VERIFY_POLICY_MASK) are the opt-in strict rules; the mode is what the other bits say. */
void eddsa_amd_set_offcurve_mode(int exact)
{
    pthread_rwlock_wrlock(&g_table);
    const int mode = exact & ~EDDSA_AMD_VERIFY_POLICY_MASK;
    g_offcurve_mode = mode == 2 ? 2 : mode != 0;
    g_verify_policy = exact & EDDSA_AMD_VERIFY_POLICY_MASK;
    pthread_rwlock_unlock(&g_table);
}

/* The equation an item is held to (include/eddsa_amd.h): a call of its own, not a bit of the word above - the policy mask and
 * the meaning of that word's other values stay what they are.  Read where a pass is enqueued, under the same lock. */
int eddsa_amd_set_verify_equation(int equation)
{
    if (equation != EDDSA_AMD_EQUATION_COFACTORLESS && equation != EDDSA_AMD_EQUATION_COFACTORED) return -(int)hipErrorInvalidValue;
    pthread_rwlock_wrlock(&g_table);
    g_verify_equation = equation;
    pthread_rwlock_unlock(&g_table);
    return 0;
}

/* The off-curve mode a pass runs in.  Under the cofactored equation a key that is no curve point is rejected whatever the
 * mode says, so mode 1 runs as mode 0 - the exact chain is not launched; the self-check mode 2 keeps its meaning. */
static int pass_offcurve_mode(void)
{
    return g_verify_equation && g_offcurve_mode == 1 ? 0 : g_offcurve_mode;
}

/* ed25519_verify_batch_rlc[_dev] calls of fewer than `items` items use the per-item kernels (default EDDSA_AMD_RLC_MIN_ITEMS_DEFAULT:
 * above the measured break-even; 0 = always try the combination) */
void eddsa_amd_set_rlc_min_items(size_t items)
{
    pthread_rwlock_wrlock(&g_table);
    g_rlc_min_items = items;
    pthread_rwlock_unlock(&g_table);
}

/* ------------------------------------------------------------------------------------------
 * device-pointer work on one engine (the engine's device is current)
 * ---------------------------------------------------------------------------------------- */

/* a pass failed half-way: kernels already queued may still use the slot; wait for them before the
 * slot can be handed out (and possibly re-allocated) again */
static void slot_quiesce(struct vslot *v, hipStream_t st)
{
    HIP_NOTE(hipStreamSynchronize(st));
    if (v->ws.side) HIP_NOTE(hipStreamSynchronize(v->ws.side));
    HIP_NOTE(hipEventRecord(v->free, st));
}

int take_async_error(struct engine *e)
{
    return __atomic_exchange_n(e->status, 0u, __ATOMIC_ACQ_REL) == EDK_STATUS_STALLED ? EDDSA_AMD_STALLED : 0;
}

/* A workspace pass: the chunks of one call, at most CHUNK_MAX items each, through one slot of the pool on stream `st`.
 * pass_open takes e->lk, picks the slot, grows the workspaces named in `what` to the call's largest chunk and orders the
 * stream behind the slot's previous pass (closing the pass itself if that fails); pass_close records the slot free behind
 * the pass - or, after an error, waits for what was queued - and drops the lock.  The caller queues its chunks in between. */
enum { PASS_WS = 1, PASS_RWS = 2, PASS_FWS = 4,
       PASS_BUSY = 8 };   /* the caller drops e->lk inside the pass: the slot is marked busy, which ws_pick honours */
struct pass { struct engine *e; struct vslot *v; hipStream_t st; int queued; };

static int pass_close(struct pass *p, int rc)
{
    if (p->queued && !rc) rc = -(int)hipEventRecord(p->v->free, p->st);
    if (p->queued && rc) slot_quiesce(p->v, p->st);   /* (a failed reserve has queued nothing) */
    if (p->v->busy) { p->v->busy = 0; pthread_cond_broadcast(&p->e->slot_cv); }
    pthread_mutex_unlock(&p->e->lk);
    return rc;
}

static int pass_open(struct pass *p, struct engine *e, size_t n, int what, hipStream_t st)
{
    int rc = 0;
    const size_t items = n < CHUNK_MAX ? n : CHUNK_MAX;
    pthread_mutex_lock(&e->lk);
    *p = (struct pass){ e, ws_pick(e, st), st, 0 };
    p->v->busy = (what & PASS_BUSY) != 0;
    if (what & PASS_WS) rc = ws_reserve(p->v, items);
    if (!rc && (what & PASS_RWS)) rc = rws_reserve(p->v, items);
    if (!rc && (what & PASS_FWS)) rc = fws_reserve(p->v, items, st);
    p->queued = !rc;
    if (!rc) rc = -(int)hipStreamWaitEvent(st, p->v->free, 0);   /* the slot may have served another stream: behind its previous pass */
    return rc ? pass_close(p, rc) : 0;
}

/* what the pass that starts at item `done` of a call of n items reads */
static edk_verify_src src_at(const edk_verify_src *all, size_t n, size_t done)
{
    edk_verify_src src = *all;
    if (all->msg_off && !all->msg_end) src.msg_end = all->msg_off + n;   /* the kernels clamp every span into [0, msg_off[n]) */
    if (all->sc_data) {   /* scattered: the chunk's four index arrays; its packed arrays are the workspace's (verify_on) */
        src.sc_sig_off += done; src.sc_pub_off += done; src.sc_msg_off += done; src.sc_msg_len += done;
    } else {
        src.sigs += done * all->sig_stride;
        if (all->pubs) src.pubs += done * all->pub_stride;   /* (a keyed pass has none) */
        if (all->msg_off) src.msg_off += done; else src.msgs += done * all->msg_stride;
    }
    if (all->key_idx) src.key_idx += done;   /* keyed passes: the chunk's indices are the chunk's */
    src.policy = g_verify_policy;   /* read where the pass is enqueued, like g_offcurve_mode */
    src.equation = g_verify_equation;
    return src;
}

/* edk_scatter_challenge is a WEAK reference (edk_scatter.h), like edk_point_classify and edk_point_muladd further down */
extern __typeof__(edk_scatter_challenge) edk_scatter_challenge __attribute__((weak));
extern __typeof__(edk_scatter_spans_inside) edk_scatter_spans_inside __attribute__((weak));

/* caller holds e->lk, inside a pass on the slot: the area the front kernel of a scattered pass gathers the signatures into, 64 bytes
 * per item of the slot's capacity.  Only a slot that serves such a pass ever holds one; ws_release frees it with the slot's other
 * buffers, so one that exists fits the capacity.  (Fresh memory: nothing that is queued on the slot uses it.) */
static hipError_t gsigs_reserve(struct vslot *v)
{
    return v->ws.gsigs ? hipSuccess : hipMalloc((void **)&v->ws.gsigs, v->ws.capacity * 64);
}

/* both verify forms */
int verify_on(struct engine *e, uint8_t *ok, const edk_verify_src *all, size_t n, hipStream_t st, hipEvent_t bulk_done, int bulk_early)
{
    int rc = 0;
    struct pass p;
    if (n == 0) return 0;
    if ((rc = take_async_error(e))) return rc;   /* an earlier pass's kernels gave up: see engine.h */
    if (all->sc_data && !edk_scatter_challenge) return -(int)hipErrorNotSupported;
    if ((rc = pass_open(&p, e, n, PASS_WS, st))) return rc;
    if (all->sc_data) TRY(gsigs_reserve(p.v));
    p.v->ws.exact_offcurve = pass_offcurve_mode();
    p.v->ws.comb = e->comb;
    p.v->ws.algo = p.v->ws.exact_offcurve ? g_verify_algo : 1;   /* the reject mode has no exact path for the items the pair search gives up on */
    for (size_t done = 0; done < n; done += CHUNK_MAX) {
        const size_t m = n - done < CHUNK_MAX ? n - done : CHUNK_MAX;
        edk_verify_src src = src_at(all, n, done);
        hipEvent_t *marks = NULL;
        if (g_profiling && e->marks_used < MARK_SLOTS) marks = e->marks[e->marks_used++];
        if (src.sc_data) {   /* scattered: gather and hash in front, then the digest pass over what that left in the slot */
            TRY(edk_scatter_challenge(src.sc_data, src.sc_data_len, src.sc_sig_off, src.sc_pub_off, src.sc_msg_off, src.sc_msg_len, m,
                                      &p.v->ws, st));
            src.sigs = p.v->ws.gsigs; src.pubs = p.v->ws.keybytes; src.msgs = p.v->ws.domdig;
        }
        TRY(edk_verify(ok + done, &src, m, e->base16, &p.v->ws, marks, done + CHUNK_MAX >= n ? bulk_done : NULL, bulk_early, st));
    }
out:
    return pass_close(&p, rc);
}

/* the fixed-base operations and x25519 share one driver */
typedef hipError_t (*fixed_step)(struct engine *e, size_t done, size_t m, const void *ctx, const edk_fixed_ws *fws, hipStream_t st);

static int fixed_on(struct engine *e, size_t n, fixed_step step, const void *ctx, hipStream_t st)
{
    int rc = 0;
    struct pass p;
    if (n == 0) return 0;
    if ((rc = pass_open(&p, e, n, PASS_FWS, st))) return rc;
    for (size_t done = 0; done < n; done += CHUNK_MAX)
        TRY(step(e, done, n - done < CHUNK_MAX ? n - done : CHUNK_MAX, ctx, &p.v->fws, st));
out:
    return pass_close(&p, rc);
}

/* set NULL: `first` holds the secret keys and pubs the public ones; else `first` holds the key indices into the signer set */
struct sign_ctx { uint8_t *sigs; const edk_signer_set *set; const uint8_t *first, *pubs, *msgs; const uint64_t *msg_off, *msg_end; size_t msg_len;
                  const edk_dom *dom; };

/* edk_sign_keyed is a WEAK reference (edk_signer.h): without the HIP translation unit no signer set can exist, so no pass gets here */
extern __typeof__(edk_signer_build) edk_signer_build __attribute__((weak));
extern __typeof__(edk_sign_keyed) edk_sign_keyed __attribute__((weak));

static hipError_t sign_step(struct engine *e, size_t done, size_t m, const void *vctx, const edk_fixed_ws *fws, hipStream_t st)
{
    const struct sign_ctx *c = (const struct sign_ctx *)vctx;
    const uint8_t *mp = c->msg_off ? c->msgs : c->msgs + done * c->msg_len;
    const uint64_t *op = c->msg_off ? c->msg_off + done : NULL;
    edk_fixed_ws with_dom = *fws;                  /* Ed25519ctx / Ed25519ph: the prefix travels in the launcher's copy of the workspace */
    with_dom.dom = c->dom;
    if (!c->set)
        return edk_sign(c->sigs + 64 * done, c->first + 32 * done, c->pubs + 32 * done, mp, op, c->msg_end, c->msg_len, m,
                        e->comb_img, &with_dom, st);
    if (!edk_sign_keyed) return hipErrorNotSupported;
    return edk_sign_keyed(c->sigs + 64 * done, c->set, (const uint32_t *)c->first + done, mp, op, c->msg_end, c->msg_len, m,
                          e->comb_img, &with_dom, st);
}

struct io_ctx { uint8_t *out; const uint8_t *in; };
struct io2_ctx { uint8_t *out; const uint8_t *a, *b; };

static hipError_t genpub_step(struct engine *e, size_t done, size_t m, const void *vctx, const edk_fixed_ws *fws, hipStream_t st)
{
    const struct io_ctx *c = (const struct io_ctx *)vctx;
    return edk_genpub(c->out + 32 * done, c->in + 32 * done, m, e->comb_img, fws, st);
}

static hipError_t x25519_step(struct engine *e, size_t done, size_t m, const void *vctx, const edk_fixed_ws *fws, hipStream_t st)
{
    const struct io2_ctx *c = (const struct io2_ctx *)vctx;
    (void)e;
    return edk_x25519(c->out + 32 * done, c->a + 32 * done, c->b + 32 * done, m, fws, st);
}

static hipError_t xbase_step(struct engine *e, size_t done, size_t m, const void *vctx, const edk_fixed_ws *fws, hipStream_t st)
{
    const struct io_ctx *c = (const struct io_ctx *)vctx;
    return edk_x25519_base(c->out + 32 * done, c->in + 32 * done, m, e->comb_img, fws, st);
}

/* every sign form (engine.h) */
int sign_on(struct engine *e, uint8_t *sigs, const eddsa_amd_signer *sg, const uint8_t *first, const uint8_t *pubs, const uint8_t *msgs,
            const uint64_t *msg_off, size_t msg_len, size_t n, const edk_dom *dom, hipStream_t st)
{
    struct sign_ctx c = { .sigs = sigs, .set = sg ? &sg->set : NULL, .first = first, .pubs = pubs, .msgs = msgs, .msg_off = msg_off,
                          .msg_end = msg_off ? msg_off + n : NULL, .msg_len = msg_len, .dom = dom };   /* spans are clamped into [0, msg_off[n]) */
    return fixed_on(e, n, sign_step, &c, st);
}

/* dom2(flag, context) of RFC 8032 section 2 as the kernels take it (eddsa_kernels.h: edk_dom); a context of more than 255 bytes,
 * or none where a length is given, is refused */
int dom2_fill(edk_dom *d, int flag, const uint8_t *context, size_t context_len)
{
    static const char tag[32 + 1] = "SigEd25519 no Ed25519 collisions";
    uint8_t bytes[EDK_DOM_WORDS * 4];
    if (context_len > EDK_DOM_CONTEXT_MAX || (context_len && !context)) return -(int)hipErrorInvalidValue;
    memset(bytes, 0, sizeof(bytes));
    memcpy(bytes, tag, 32);
    bytes[32] = (uint8_t)flag;
    bytes[33] = (uint8_t)context_len;
    if (context_len) memcpy(bytes + EDK_DOM_FIXED_BYTES, context, context_len);
    d->len = (uint32_t)(EDK_DOM_FIXED_BYTES + context_len);
    for (int k = 0; k < EDK_DOM_WORDS; k++)
        d->w[k] = (uint32_t)bytes[4 * k] | (uint32_t)bytes[4 * k + 1] << 8 | (uint32_t)bytes[4 * k + 2] << 16 | (uint32_t)bytes[4 * k + 3] << 24;
    return 0;
}

int genpub_on(struct engine *e, uint8_t *pubs, const uint8_t *secs, size_t n, hipStream_t st)
{
    struct io_ctx x = { pubs, secs };
    return fixed_on(e, n, genpub_step, &x, st);
}

int x25519_on(struct engine *e, uint8_t *out, const uint8_t *scalars, const uint8_t *points, size_t n, hipStream_t st)
{
    struct io2_ctx x = { out, scalars, points };
    return fixed_on(e, n, x25519_step, &x, st);
}

int xbase_on(struct engine *e, uint8_t *out, const uint8_t *scalars, size_t n, hipStream_t st)
{
    struct io_ctx x = { out, scalars };
    return fixed_on(e, n, xbase_step, &x, st);
}

int pk_to_x_on(struct engine *e, uint8_t *out, const uint8_t *in, size_t n, hipStream_t st)
{
    (void)e;
    hipError_t er = edk_pk_to_x(out, in, n, st);
    return er == hipSuccess ? 0 : -(int)er;
}

int sk_to_x_on(struct engine *e, uint8_t *out, const uint8_t *in, size_t n, hipStream_t st)
{
    (void)e;
    hipError_t er = edk_sk_to_x(out, in, n, st);
    return er == hipSuccess ? 0 : -(int)er;
}

/* edk_point_classify is a WEAK reference (edk_classify.h), like edk_signer_build: the host side is also linked without the HIP
 * translation unit (tests/fake_hip) - classifying is then hipErrorNotSupported */
extern __typeof__(edk_point_classify) edk_point_classify __attribute__((weak));

int classify_on(struct engine *e, uint8_t *cls, const uint8_t *points, size_t n, hipStream_t st)
{
    (void)e;
    if (!edk_point_classify) return -(int)hipErrorNotSupported;
    hipError_t er = edk_point_classify(cls, points, n, st);
    return er == hipSuccess ? 0 : -(int)er;
}

/* edk_point_muladd is a WEAK reference (edk_muladd.h), like edk_point_classify */
extern __typeof__(edk_point_muladd) edk_point_muladd __attribute__((weak));

/* [m]P + [a]B (include/eddsa_amd.h: ed25519_point_muladd_batch*): chunks of at most CHUNK_MAX items through one slot of the verify
 * workspace pool, as verify_on walks them - the pass orders itself behind and in front of verify passes on the same slot through the
 * slot's `free` event (pass_open, pass_close).  It runs k_verify_main over its own digits and table and has no exact path, so it
 * reports nothing itself; an earlier verify pass's report is taken here as in verify_on */
int muladd_on(struct engine *e, uint8_t *out, const uint8_t *points, const uint8_t *mul, const uint8_t *add, size_t n, hipStream_t st)
{
    int rc = 0;
    struct pass p;
    if (n == 0) return 0;
    if (!edk_point_muladd) return -(int)hipErrorNotSupported;
    if ((rc = take_async_error(e))) return rc;
    if ((rc = pass_open(&p, e, n, PASS_WS, st))) return rc;
    for (size_t done = 0; done < n; done += CHUNK_MAX) {
        const size_t m = n - done < CHUNK_MAX ? n - done : CHUNK_MAX;
        TRY(edk_point_muladd(out + 32 * done, points + 32 * done, mul ? mul + 32 * done : NULL, add ? add + 32 * done : NULL, m, e->base16,
                             &p.v->ws, st));
    }
out:
    return pass_close(&p, rc);
}

/* Batch verification by random linear combination (reference lib/ed25519-sha512.c:13-14, its TODO;
 * SURVEY 8(f)-3): see include/eddsa_amd.h.  One pass of at most CHUNK_MAX items; larger batches are
 * split into independent sub-batches. */
int rlc_on(struct engine *e, uint8_t *ok, uint32_t *stats, const edk_verify_src *all, size_t n, hipStream_t st)
{
    int rc = 0;
    struct pass p;
    if (n == 0) return 0;
    if (n < g_rlc_min_items || (all->ks_table && all->ks_count > EDK_RLC_MAX_KEYS)) {
        /* the combination has about 1 ms of latency of its own (hash tree, one serial Horner per group): below
         * ~2^17 items the per-item kernels are faster (tools/rlc_sizes.py), so such calls go straight to them - a keyed call
         * (all->ks_table) to the keyed ones, and so does every call over a key set wider than a group */
        rc = verify_on(e, ok, all, n, st, NULL, 0);
        if (!rc) { hipError_t er = edk_rlc_note_per_item(stats, n, st); if (er != hipSuccess) rc = -(int)er; }
        return rc;
    }
    if ((rc = take_async_error(e))) return rc;
    /* The combination's group verdicts are read by the host, once per pass.  The wait for the stream happens OUTSIDE
     * e->lk (other threads keep enqueueing on this engine meanwhile); the workspace slot stays reserved through its
     * busy mark, which ws_pick honours. */
    if ((rc = pass_open(&p, e, n, PASS_WS | PASS_RWS | PASS_BUSY, st))) return rc;
    /* (the fallback of the cofactorless equation always has the exact path; under the cofactored one it rejects off-curve keys
     * like every pass, and verify_route_of takes the full-length route) */
    p.v->ws.exact_offcurve = g_verify_equation ? pass_offcurve_mode() : g_offcurve_mode ? g_offcurve_mode : 1;
    p.v->ws.algo = g_verify_algo;
    p.v->ws.comb = e->comb;   /* groups sent to the per-item kernels over a comb key set take the comb route */
    for (size_t done = 0; done < n; done += CHUNK_MAX) {
        const size_t m = n - done < CHUNK_MAX ? n - done : CHUNK_MAX;
        const edk_verify_src src = src_at(all, n, done);
        TRY(edk_verify_rlc(ok + done, stats, &src, m, e->base16, &p.v->ws, &p.v->rws, st));
#ifdef EDDSA_AMD_DEBUG_BUILD
        e->snap_slot = (int)(p.v - e->vs); e->snap_n = m;   /* what eddsa_amd_debug_rlc_snapshot reads */
#endif
        pthread_mutex_unlock(&e->lk);
        hipError_t er = hipStreamSynchronize(st);
        pthread_mutex_lock(&e->lk);
        TRY(er);
        TRY(edk_verify_rlc_fallback(ok + done, &src, m, e->base16, &p.v->ws, &p.v->rws, st));
    }
out:
    return pass_close(&p, rc);
}

/* ------------------------------------------------------------------------------------------
 * device-pointer entry points: run on the device that holds the output buffer (an empty batch
 * is done before that pointer is looked at)
 * ---------------------------------------------------------------------------------------- */

static int enter_dev(struct call *c, const void *out)
{
    int dev = -1;
    const int rc = device_of(out, &dev);
    return rc ? rc : enter(c, dev);
}

/* return leave_with(&c, work(c.e, ..)): the work's answer, after leave() */
static int leave_with(struct call *c, int rc) { leave(c); return rc; }

/* fixed-size records: see include/eddsa_amd.h */
int records_ok(size_t stride, size_t sig_off, size_t pub_off, size_t msg_off, size_t msg_len)
{
    return sig_off <= stride && 64 <= stride - sig_off && pub_off <= stride && 32 <= stride - pub_off &&
           msg_off <= stride && msg_len <= stride - msg_off;
}

/* the checks that every verify and sign form makes before any device is asked (engine.h) */
int msg_call_open(const struct msg_call *c, edk_dom *dom_buf, const edk_dom **dom)
{
    *dom = NULL;
    if (c->ctx) {                          /* (the prefix is built first: a context of more than 255 bytes ends the call before anything else is looked at) */
        const int rc = dom2_fill(dom_buf, c->ctx - 1, c->context, c->context_len);
        if (rc) return rc;
        *dom = dom_buf;
    }
    if (c->records && !records_ok(c->stride, c->rec_sig, c->rec_pub, c->rec_msg, c->msg_len)) return -(int)hipErrorInvalidValue;
    if (c->keyed && !c->ks && !c->sg) return -(int)hipErrorInvalidValue;
    if (c->n == 0) return 1;
    if (c->keyed && (!c->out || !c->first || (c->ks && !c->second) || (!c->msgs && c->msg_len && !c->msg_off)))
        return -(int)hipErrorInvalidValue;   /* (fixed-length items need their buffer) */
    return 0;
}

/* The one body of the device-pointer verify and sign forms: the shared checks, then the device of the output buffer - which for a
 * keyed form must be the one its key set's tables / its signer set's secrets live on -, then the pass.  The prefix of ctx / ph is
 * built here, on the host, and goes to the kernels by value. */
static int msg_call_dev(const struct msg_call *c, int sign, void *stream)
{
    edk_dom dom_buf;
    const edk_dom *dom;
    struct call e;
    int dev = -1, rc = msg_call_open(c, &dom_buf, &dom);
    if (rc) return rc < 0 ? rc : 0;
    if ((rc = device_of(c->out, &dev))) return rc;
    if (c->keyed && dev != (c->ks ? c->ks->device : c->sg->device)) return -(int)hipErrorInvalidValue;
    if ((rc = enter(&e, dev))) return rc;
    if (sign) {
        rc = sign_on(e.e, c->out, c->sg, c->first, c->second, c->msgs, c->msg_off, c->msg_len, c->n, dom, (hipStream_t)stream);
    } else {
        const struct verify_form f = { .ks = c->ks, .digest = c->digest, .dom = dom, .rlc = c->rlc };
        const edk_verify_src src = c->records ? verify_src_records(c->first, c->stride, c->rec_sig, c->rec_pub, c->rec_msg, c->msg_len)
                                              : verify_src(&f, c->first, c->second, c->msgs, c->msg_off, c->msg_len);
        rc = f.rlc ? rlc_on(e.e, c->out, c->stats, &src, c->n, (hipStream_t)stream)
                   : verify_on(e.e, c->out, &src, c->n, (hipStream_t)stream, NULL, 0);
    }
    leave(&e);
    return rc;
}

/* the eleven verify forms: argument adapters */
int ed25519_verify_batch_dev(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs, const uint8_t *msgs,
                             const uint64_t *msg_off, size_t msg_len, size_t n, void *stream)
{
    const struct msg_call c = { .out = ok, .first = sigs, .second = pubs, .msgs = msgs, .msg_off = msg_off, .msg_len = msg_len, .n = n };
    return msg_call_dev(&c, 0, stream);
}

int ed25519_verify_records_dev(uint8_t *ok, const uint8_t *records, size_t stride, size_t sig_off, size_t pub_off,
                               size_t msg_off, size_t msg_len, size_t n, void *stream)
{
    const struct msg_call c = { .out = ok, .first = records, .msg_len = msg_len, .n = n,
                                .records = 1, .stride = stride, .rec_sig = sig_off, .rec_pub = pub_off, .rec_msg = msg_off };
    return msg_call_dev(&c, 0, stream);
}

int ed25519_verify_batch_rlc_dev(uint8_t *ok, uint32_t *stats, const uint8_t *sigs, const uint8_t *pubs,
                                 const uint8_t *msgs, const uint64_t *msg_off, size_t msg_len, size_t n, void *stream)
{
    const struct msg_call c = { .out = ok, .stats = stats, .first = sigs, .second = pubs, .msgs = msgs, .msg_off = msg_off, .msg_len = msg_len,
                                .n = n, .rlc = 1 };
    return msg_call_dev(&c, 0, stream);
}

/* caller-supplied digests (include/eddsa_amd.h): the two calls above with the 64 bytes of SHA-512(R || A || M) per item in the
 * message slot and the flag that selects the kernels that do not hash */
int ed25519_verify_digests_dev(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs, const uint8_t *digests, size_t n, void *stream)
{
    const struct msg_call c = { .out = ok, .first = sigs, .second = pubs, .msgs = digests, .msg_len = EDDSA_DIGEST_BYTES, .n = n, .digest = 1 };
    return msg_call_dev(&c, 0, stream);
}

int ed25519_verify_digests_rlc_dev(uint8_t *ok, uint32_t *stats, const uint8_t *sigs, const uint8_t *pubs, const uint8_t *digests,
                                   size_t n, void *stream)
{
    const struct msg_call c = { .out = ok, .stats = stats, .first = sigs, .second = pubs, .msgs = digests, .msg_len = EDDSA_DIGEST_BYTES, .n = n,
                                .digest = 1, .rlc = 1 };
    return msg_call_dev(&c, 0, stream);
}

/* Ed25519ctx and Ed25519ph (include/eddsa_amd.h): the message forms with dom2(F, context) in front of the hash; ph is ctx with
 * F = 1 over the caller's 64-byte prehashes */
int ed25519ctx_verify_batch_dev(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs, const uint8_t *msgs, const uint64_t *msg_off,
                                size_t msg_len, size_t n, const uint8_t *context, size_t context_len, void *stream)
{
    const struct msg_call c = { .out = ok, .first = sigs, .second = pubs, .msgs = msgs, .msg_off = msg_off, .msg_len = msg_len, .n = n,
                                .ctx = CTX_ED25519CTX, .context = context, .context_len = context_len };
    return msg_call_dev(&c, 0, stream);
}

int ed25519ph_verify_batch_dev(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs, const uint8_t *prehashes, size_t n,
                               const uint8_t *context, size_t context_len, void *stream)
{
    const struct msg_call c = { .out = ok, .first = sigs, .second = pubs, .msgs = prehashes, .msg_len = EDDSA_PREHASH_BYTES, .n = n,
                                .ctx = CTX_ED25519PH, .context = context, .context_len = context_len };
    return msg_call_dev(&c, 0, stream);
}

/* ------------------------------------------------------------------------------------------
 * key sets (include/eddsa_amd.h): keys registered once, verified against by index
 * ---------------------------------------------------------------------------------------- */

/* edk_keyset_build is a WEAK reference, like edk_rlc_region below: the host side is also linked without the HIP translation
 * unit (tests/fake_hip) - creating a key set is then hipErrorNotSupported */
extern __typeof__(edk_keyset_build) edk_keyset_build __attribute__((weak));
extern __typeof__(edk_keyset_comb_build) edk_keyset_comb_build __attribute__((weak));

static void keyset_free(eddsa_amd_keyset *ks)
{
    if (ks->keys) HIP_NOTE(hipFree(ks->keys));
    if (ks->flags) HIP_NOTE(hipFree(ks->flags));
    if (ks->table) HIP_NOTE(hipFree(ks->table));
    if (ks->comb) HIP_NOTE(hipFree(ks->comb));
    free(ks);
}

/* device < 0: host keys, on the default device; else device keys on `device`.  comb != 0: a comb key set - everything a plain one
 * holds, and KEYSET_COMB_WORDS words per key on top.  Returns once the tables are built. */
static int keyset_create_on(eddsa_amd_keyset **out, const uint8_t *keys, size_t count, int device, hipStream_t st, int comb)
{
    struct call c;
    int rc;
    eddsa_amd_keyset *ks;
    if (!edk_keyset_build || (comb && !edk_keyset_comb_build)) return -(int)hipErrorNotSupported;
    if ((rc = enter(&c, device))) return rc;
    ks = (eddsa_amd_keyset *)calloc(1, sizeof(*ks));
    if (!ks) { rc = -(int)hipErrorOutOfMemory; goto out; }
    ks->device = c.e->device;
    ks->count = count;
    TRY(hipMalloc((void **)&ks->keys, count * 32));
    TRY(hipMalloc((void **)&ks->flags, count));
    TRY(hipMalloc((void **)&ks->table, count * VERIFY_ITEM_TABLE_WORDS * sizeof(uint32_t)));
    TRY(hipMemcpyAsync(ks->keys, keys, count * 32, device < 0 ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    ks->bytes = count * (32 + 1 + VERIFY_ITEM_TABLE_WORDS * sizeof(uint32_t));
    if (comb) {
        TRY(hipMalloc((void **)&ks->comb, count * KEYSET_COMB_WORDS * sizeof(uint32_t)));
        ks->bytes += count * KEYSET_COMB_WORDS * sizeof(uint32_t);
    }
    TRY(edk_keyset_build(ks->table, ks->flags, ks->keys, count, st));
    if (comb) TRY(edk_keyset_comb_build(ks->comb, ks->keys, count, st));
    TRY(hipStreamSynchronize(st));
    *out = ks;
    ks = NULL;
out:
    if (ks) { HIP_NOTE(hipStreamSynchronize(st)); keyset_free(ks); }
    leave(&c);
    return rc;
}

/* the four entry points: *out is NULL after every failure; limit: the most keys a set of this kind may hold (a comb key set: 88 KiB
 * of HBM per key); on_device: `keys` lies in HBM and the set is built on its device, else on the default one */
static int keyset_create_checked(eddsa_amd_keyset **out, const uint8_t *keys, size_t count, size_t limit, int on_device, void *stream, int comb)
{
    int dev = -1, rc;
    if (out) *out = NULL;
    if (!out || !keys || count == 0 || count > limit) return -(int)hipErrorInvalidValue;
    if (on_device && (rc = device_of(keys, &dev))) return rc;
    return keyset_create_on(out, keys, count, dev, (hipStream_t)stream, comb);
}

int eddsa_amd_keyset_create(eddsa_amd_keyset **out, const uint8_t *keys, size_t count)
{
    return keyset_create_checked(out, keys, count, EDDSA_AMD_KEYSET_MAX_KEYS, 0, NULL, 0);
}

int eddsa_amd_keyset_create_dev(eddsa_amd_keyset **out, const uint8_t *keys, size_t count, void *stream)
{
    return keyset_create_checked(out, keys, count, EDDSA_AMD_KEYSET_MAX_KEYS, 1, stream, 0);
}

int eddsa_amd_keyset_create_comb(eddsa_amd_keyset **out, const uint8_t *keys, size_t count)
{
    return keyset_create_checked(out, keys, count, EDDSA_AMD_KEYSET_COMB_MAX_KEYS, 0, NULL, 1);
}

int eddsa_amd_keyset_create_comb_dev(eddsa_amd_keyset **out, const uint8_t *keys, size_t count, void *stream)
{
    return keyset_create_checked(out, keys, count, EDDSA_AMD_KEYSET_COMB_MAX_KEYS, 1, stream, 1);
}

void eddsa_amd_keyset_destroy(eddsa_amd_keyset *ks)
{
    int saved = -1;
    if (!ks) return;
    HIP_NOTE(hipGetDevice(&saved));
    HIP_NOTE(hipSetDevice(ks->device));
    HIP_NOTE(hipDeviceSynchronize());      /* passes that read the set may still be queued */
    keyset_free(ks);
    if (saved >= 0) HIP_NOTE(hipSetDevice(saved));
}

size_t eddsa_amd_keyset_count(const eddsa_amd_keyset *ks) { return ks ? ks->count : 0; }
int eddsa_amd_keyset_device(const eddsa_amd_keyset *ks) { return ks ? ks->device : -1; }
int eddsa_amd_keyset_is_comb(const eddsa_amd_keyset *ks) { return ks && ks->comb ? 1 : 0; }
size_t eddsa_amd_keyset_bytes(const eddsa_amd_keyset *ks) { return ks ? ks->bytes : 0; }

/* the six verify forms over a key set: the unkeyed form of the same name with the key indices where that has the keys */
int ed25519_verify_keyed_dev(uint8_t *ok, const eddsa_amd_keyset *ks, const uint32_t *key_idx, const uint8_t *sigs,
                             const uint8_t *msgs, const uint64_t *msg_off, size_t msg_len, size_t n, void *stream)
{
    const struct msg_call c = { .out = ok, .first = sigs, .second = (const uint8_t *)key_idx, .msgs = msgs, .msg_off = msg_off, .msg_len = msg_len,
                                .n = n, .keyed = 1, .ks = ks };
    return msg_call_dev(&c, 0, stream);
}

int ed25519_verify_keyed_rlc_dev(uint8_t *ok, uint32_t *stats, const eddsa_amd_keyset *ks, const uint32_t *key_idx, const uint8_t *sigs,
                                 const uint8_t *msgs, const uint64_t *msg_off, size_t msg_len, size_t n, void *stream)
{
    const struct msg_call c = { .out = ok, .stats = stats, .first = sigs, .second = (const uint8_t *)key_idx, .msgs = msgs, .msg_off = msg_off,
                                .msg_len = msg_len, .n = n, .keyed = 1, .ks = ks, .rlc = 1 };
    return msg_call_dev(&c, 0, stream);
}

int ed25519_verify_keyed_digests_dev(uint8_t *ok, const eddsa_amd_keyset *ks, const uint32_t *key_idx, const uint8_t *sigs,
                                     const uint8_t *digests, size_t n, void *stream)
{
    const struct msg_call c = { .out = ok, .first = sigs, .second = (const uint8_t *)key_idx, .msgs = digests, .msg_len = EDDSA_DIGEST_BYTES,
                                .n = n, .keyed = 1, .ks = ks, .digest = 1 };
    return msg_call_dev(&c, 0, stream);
}

int ed25519_verify_keyed_digests_rlc_dev(uint8_t *ok, uint32_t *stats, const eddsa_amd_keyset *ks, const uint32_t *key_idx,
                                         const uint8_t *sigs, const uint8_t *digests, size_t n, void *stream)
{
    const struct msg_call c = { .out = ok, .stats = stats, .first = sigs, .second = (const uint8_t *)key_idx, .msgs = digests,
                                .msg_len = EDDSA_DIGEST_BYTES, .n = n, .keyed = 1, .ks = ks, .digest = 1, .rlc = 1 };
    return msg_call_dev(&c, 0, stream);
}

int ed25519ctx_verify_keyed_dev(uint8_t *ok, const eddsa_amd_keyset *ks, const uint32_t *key_idx, const uint8_t *sigs, const uint8_t *msgs,
                                const uint64_t *msg_off, size_t msg_len, size_t n, const uint8_t *context, size_t context_len, void *stream)
{
    const struct msg_call c = { .out = ok, .first = sigs, .second = (const uint8_t *)key_idx, .msgs = msgs, .msg_off = msg_off, .msg_len = msg_len,
                                .n = n, .keyed = 1, .ks = ks, .ctx = CTX_ED25519CTX, .context = context, .context_len = context_len };
    return msg_call_dev(&c, 0, stream);
}

int ed25519ph_verify_keyed_dev(uint8_t *ok, const eddsa_amd_keyset *ks, const uint32_t *key_idx, const uint8_t *sigs,
                               const uint8_t *prehashes, size_t n, const uint8_t *context, size_t context_len, void *stream)
{
    const struct msg_call c = { .out = ok, .first = sigs, .second = (const uint8_t *)key_idx, .msgs = prehashes, .msg_len = EDDSA_PREHASH_BYTES,
                                .n = n, .keyed = 1, .ks = ks, .ctx = CTX_ED25519PH, .context = context, .context_len = context_len };
    return msg_call_dev(&c, 0, stream);
}

/* the three sign forms over caller-supplied keys; those over a signer set stand behind the signer sets */
int ed25519_sign_batch_dev(uint8_t *sigs, const uint8_t *secs, const uint8_t *pubs, const uint8_t *msgs,
                           const uint64_t *msg_off, size_t msg_len, size_t n, void *stream)
{
    const struct msg_call c = { .out = sigs, .first = secs, .second = pubs, .msgs = msgs, .msg_off = msg_off, .msg_len = msg_len, .n = n };
    return msg_call_dev(&c, 1, stream);
}

int ed25519ctx_sign_batch_dev(uint8_t *sigs, const uint8_t *secs, const uint8_t *pubs, const uint8_t *msgs, const uint64_t *msg_off,
                              size_t msg_len, size_t n, const uint8_t *context, size_t context_len, void *stream)
{
    const struct msg_call c = { .out = sigs, .first = secs, .second = pubs, .msgs = msgs, .msg_off = msg_off, .msg_len = msg_len, .n = n,
                                .ctx = CTX_ED25519CTX, .context = context, .context_len = context_len };
    return msg_call_dev(&c, 1, stream);
}

int ed25519ph_sign_batch_dev(uint8_t *sigs, const uint8_t *secs, const uint8_t *pubs, const uint8_t *prehashes, size_t n,
                             const uint8_t *context, size_t context_len, void *stream)
{
    const struct msg_call c = { .out = sigs, .first = secs, .second = pubs, .msgs = prehashes, .msg_len = EDDSA_PREHASH_BYTES, .n = n,
                                .ctx = CTX_ED25519PH, .context = context, .context_len = context_len };
    return msg_call_dev(&c, 1, stream);
}

/* ------------------------------------------------------------------------------------------
 * signer sets (include/eddsa_amd.h): secret keys registered once, signed with by index
 * ---------------------------------------------------------------------------------------- */

static void signer_free(eddsa_amd_signer *s)
{
    if (s->mem) wipe_free(s->mem, s->count * 64);  /* the scalars and the prefixes are zeroed on the device before the memory goes back */
    free(s);
}

/* keys: host memory, `width` bytes per key (32: seeds, 64: scalar | prefix); on the default device.  The keys are staged through a
 * device buffer that is zeroed before the call returns; the caller's memory is not page-locked and nothing else copies it. */
static int signer_create_on(eddsa_amd_signer **out, const uint8_t *keys, size_t count, size_t width)
{
    struct call c;
    int rc;
    eddsa_amd_signer *s;
    uint8_t *stage = NULL;
    if (!edk_signer_build || !edk_sign_keyed) return -(int)hipErrorNotSupported;
    if ((rc = enter(&c, -1))) return rc;
    s = (eddsa_amd_signer *)calloc(1, sizeof(*s));
    if (!s) { rc = -(int)hipErrorOutOfMemory; goto out; }
    s->device = c.e->device;
    s->count = count;
    TRY(hipMalloc((void **)&s->mem, count * 96));
    TRY(hipMalloc((void **)&stage, count * width));
    s->set.a = (const uint32_t *)s->mem;
    s->set.prefix = (const uint32_t *)(s->mem + count * 32);
    s->set.pubs = s->mem + count * 64;
    s->set.count = count;
    TRY(hipMemcpyAsync(stage, keys, count * width, hipMemcpyHostToDevice, NULL));
    TRY(edk_signer_build((uint32_t *)s->mem, (uint32_t *)(s->mem + count * 32), s->mem + count * 64, stage, count, width == 64, c.e->comb_img, NULL));
    TRY(hipStreamSynchronize(NULL));
    *out = s;
    s = NULL;
out:
    if (stage) { HIP_NOTE(hipStreamSynchronize(NULL)); wipe_free(stage, count * width); }
    if (s) signer_free(s);
    leave(&c);
    return rc;
}

int eddsa_amd_signer_create(eddsa_amd_signer **out, const uint8_t *secs, size_t count)
{
    if (out) *out = NULL;
    if (!out || !secs || count == 0 || count > EDDSA_AMD_SIGNER_MAX_KEYS) return -(int)hipErrorInvalidValue;
    return signer_create_on(out, secs, count, 32);
}

int eddsa_amd_signer_create_expanded(eddsa_amd_signer **out, const uint8_t *expanded, size_t count)
{
    if (out) *out = NULL;
    if (!out || !expanded || count == 0 || count > EDDSA_AMD_SIGNER_MAX_KEYS) return -(int)hipErrorInvalidValue;
    return signer_create_on(out, expanded, count, 64);
}

void eddsa_amd_signer_destroy(eddsa_amd_signer *s)
{
    int saved = -1;
    if (!s) return;
    HIP_NOTE(hipGetDevice(&saved));
    HIP_NOTE(hipSetDevice(s->device));
    HIP_NOTE(hipDeviceSynchronize());      /* passes that read the set may still be queued */
    signer_free(s);
    if (saved >= 0) HIP_NOTE(hipSetDevice(saved));
}

size_t eddsa_amd_signer_count(const eddsa_amd_signer *s) { return s ? s->count : 0; }
int eddsa_amd_signer_device(const eddsa_amd_signer *s) { return s ? s->device : -1; }

int eddsa_amd_signer_pubs(const eddsa_amd_signer *s, uint8_t *pubs)
{
    int saved = -1, rc = 0;
    if (!s || !pubs) return -(int)hipErrorInvalidValue;
    TRY(hipGetDevice(&saved));
    TRY(hipSetDevice(s->device));
    TRY(hipMemcpy(pubs, s->set.pubs, s->count * 32, hipMemcpyDeviceToHost));
out:
    if (saved >= 0) HIP_NOTE(hipSetDevice(saved));
    return rc;
}

/* the three device-pointer sign forms over a signer set */
int ed25519_sign_keyed_dev(uint8_t *sigs, const eddsa_amd_signer *s, const uint32_t *key_idx, const uint8_t *msgs, const uint64_t *msg_off,
                           size_t msg_len, size_t n, void *stream)
{
    const struct msg_call c = { .out = sigs, .first = (const uint8_t *)key_idx, .msgs = msgs, .msg_off = msg_off, .msg_len = msg_len, .n = n,
                                .keyed = 1, .sg = s };
    return msg_call_dev(&c, 1, stream);
}

int ed25519ctx_sign_keyed_dev(uint8_t *sigs, const eddsa_amd_signer *s, const uint32_t *key_idx, const uint8_t *msgs, const uint64_t *msg_off,
                              size_t msg_len, size_t n, const uint8_t *context, size_t context_len, void *stream)
{
    const struct msg_call c = { .out = sigs, .first = (const uint8_t *)key_idx, .msgs = msgs, .msg_off = msg_off, .msg_len = msg_len, .n = n,
                                .keyed = 1, .sg = s, .ctx = CTX_ED25519CTX, .context = context, .context_len = context_len };
    return msg_call_dev(&c, 1, stream);
}

int ed25519ph_sign_keyed_dev(uint8_t *sigs, const eddsa_amd_signer *s, const uint32_t *key_idx, const uint8_t *prehashes, size_t n,
                             const uint8_t *context, size_t context_len, void *stream)
{
    const struct msg_call c = { .out = sigs, .first = (const uint8_t *)key_idx, .msgs = prehashes, .msg_len = EDDSA_PREHASH_BYTES, .n = n,
                                .keyed = 1, .sg = s, .ctx = CTX_ED25519PH, .context = context, .context_len = context_len };
    return msg_call_dev(&c, 1, stream);
}

int ed25519_genpub_batch_dev(uint8_t *pubs, const uint8_t *secs, size_t n, void *stream)
{
    struct call c;
    int rc = 0;
    if (n == 0 || (rc = enter_dev(&c, pubs))) return rc;
    return leave_with(&c, genpub_on(c.e, pubs, secs, n, (hipStream_t)stream));
}

int x25519_batch_dev(uint8_t *out, const uint8_t *scalars, const uint8_t *points, size_t n, void *stream)
{
    struct call c;
    int rc = 0;
    if (n == 0 || (rc = enter_dev(&c, out))) return rc;
    return leave_with(&c, x25519_on(c.e, out, scalars, points, n, (hipStream_t)stream));
}

int x25519_base_batch_dev(uint8_t *out, const uint8_t *scalars, size_t n, void *stream)
{
    struct call c;
    int rc = 0;
    if (n == 0 || (rc = enter_dev(&c, out))) return rc;
    return leave_with(&c, xbase_on(c.e, out, scalars, n, (hipStream_t)stream));
}

int pk_ed25519_to_x25519_batch_dev(uint8_t *out, const uint8_t *in, size_t n, void *stream)
{
    struct call c;
    int rc = 0;
    if (n == 0 || (rc = enter_dev(&c, out))) return rc;
    return leave_with(&c, pk_to_x_on(c.e, out, in, n, (hipStream_t)stream));
}

int sk_ed25519_to_x25519_batch_dev(uint8_t *out, const uint8_t *in, size_t n, void *stream)
{
    struct call c;
    int rc = 0;
    if (n == 0 || (rc = enter_dev(&c, out))) return rc;
    return leave_with(&c, sk_to_x_on(c.e, out, in, n, (hipStream_t)stream));
}

/* point classification (include/eddsa_amd.h): an empty batch is done, NULLs are refused and a build without the kernel says so before
 * any device is asked */
int ed25519_point_classify_batch_dev(uint8_t *cls, const uint8_t *points, size_t n, void *stream)
{
    struct call c;
    int rc = 0;
    if (n == 0) return 0;
    if (!cls || !points) return -(int)hipErrorInvalidValue;
    if (!edk_point_classify) return -(int)hipErrorNotSupported;
    if ((rc = enter_dev(&c, cls))) return rc;
    return leave_with(&c, classify_on(c.e, cls, points, n, (hipStream_t)stream));
}

/* [m]P + [a]B (include/eddsa_amd.h): the same order of checks as point classification */
int ed25519_point_muladd_batch_dev(uint8_t *out, const uint8_t *points, const uint8_t *mul, const uint8_t *add, size_t n, void *stream)
{
    struct call c;
    int rc = 0;
    if (n == 0) return 0;
    if (!out || !points) return -(int)hipErrorInvalidValue;
    if (!edk_point_muladd) return -(int)hipErrorNotSupported;
    if ((rc = enter_dev(&c, out))) return rc;
    return leave_with(&c, muladd_on(c.e, out, points, mul, add, n, (hipStream_t)stream));
}

/* items by byte offsets into one buffer (include/eddsa_amd.h: ed25519_verify_scattered*).  Both forms refuse the same arguments in
 * the same order before any device is asked */
static int scattered_open(const uint8_t *ok, const uint8_t *data, size_t data_len, const uint32_t *sig_off, const uint32_t *pub_off,
                          const uint32_t *msg_off, const uint32_t *msg_len, size_t n)
{
    if (n == 0) return 1;
    if (!ok || !data || !sig_off || !pub_off || !msg_off || !msg_len) return -(int)hipErrorInvalidValue;
    if ((uint64_t)data_len > (uint64_t)UINT32_MAX) return -(int)hipErrorInvalidValue;
    if (!edk_scatter_challenge || !edk_scatter_spans_inside) return -(int)hipErrorNotSupported;
    return 0;
}

int ed25519_verify_scattered_dev(uint8_t *ok, const uint8_t *data, size_t data_len, const uint32_t *sig_off, const uint32_t *pub_off,
                                 const uint32_t *msg_off, const uint32_t *msg_len, size_t n, void *stream)
{
    struct call c;
    int rc = scattered_open(ok, data, data_len, sig_off, pub_off, msg_off, msg_len, n);
    if (rc) return rc < 0 ? rc : 0;
    int dev = -1, data_dev = -1;
    if ((rc = device_of(ok, &dev)) || (rc = device_of(data, &data_dev))) return rc;
    if (dev != data_dev) return -(int)hipErrorInvalidValue;   /* the lanes read `data` byte by byte: it lives where the pass runs */
    if ((rc = enter(&c, dev))) return rc;
    const edk_verify_src src = verify_src_scattered(data, data_len, sig_off, pub_off, msg_off, msg_len);
    return leave_with(&c, verify_on(c.e, ok, &src, n, (hipStream_t)stream, NULL, 0));
}

/* The host-pointer form: a plain wrapper, not a job of the staging pipeline - a chunk of items may refer to any byte of `data`, so
 * the whole buffer is resident before the first pass.  The arrays are checked first (a span that leaves the buffer refuses the call
 * with `ok` untouched), then everything is uploaded to the default device, the device form runs on a stream of its own, the
 * verdicts come back and every buffer is freed on every path.  The call has waited for its kernels, so it takes their report
 * itself, like every host-pointer call */
int ed25519_verify_scattered(uint8_t *ok, const uint8_t *data, size_t data_len, const uint32_t *sig_off, const uint32_t *pub_off,
                             const uint32_t *msg_off, const uint32_t *msg_len, size_t n)
{
    struct call c;
    const uint32_t *host[4] = { sig_off, pub_off, msg_off, msg_len };
    uint32_t *d_idx[4] = { NULL, NULL, NULL, NULL };
    uint8_t *d_data = NULL, *d_ok = NULL;
    hipStream_t st = NULL;
    int rc = scattered_open(ok, data, data_len, sig_off, pub_off, msg_off, msg_len, n);
    if (rc) return rc < 0 ? rc : 0;
    if (!edk_scatter_spans_inside(data_len, sig_off, pub_off, msg_off, msg_len, n)) return -(int)hipErrorInvalidValue;
    if ((rc = enter(&c, -1))) return rc;
    TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    TRY(hipMalloc((void **)&d_data, data_len ? data_len : 1));
    TRY(hipMalloc((void **)&d_ok, n));
    TRY(hipMemcpyAsync(d_data, data, data_len, hipMemcpyHostToDevice, st));
    for (int k = 0; k < 4; k++) {
        TRY(hipMalloc((void **)&d_idx[k], n * sizeof(uint32_t)));
        TRY(hipMemcpyAsync(d_idx[k], host[k], n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    {
        const edk_verify_src src = verify_src_scattered(d_data, data_len, d_idx[0], d_idx[1], d_idx[2], d_idx[3]);
        if ((rc = verify_on(c.e, d_ok, &src, n, st, NULL, 0))) goto out;
    }
    TRY(hipMemcpyAsync(ok, d_ok, n, hipMemcpyDeviceToHost, st));
    TRY(hipStreamSynchronize(st));
    rc = take_async_error(c.e);
out:
    if (st) { HIP_NOTE(hipStreamSynchronize(st)); HIP_NOTE(hipStreamDestroy(st)); }
    for (int k = 0; k < 4; k++) if (d_idx[k]) HIP_NOTE(hipFree(d_idx[k]));
    if (d_ok) HIP_NOTE(hipFree(d_ok));
    if (d_data) HIP_NOTE(hipFree(d_data));
    return leave_with(&c, rc);
}

/* The class bytes of a key set's own keys, where they lie.  No engine is asked for - the kernel reads no table and takes no workspace,
 * and the set outlives eddsa_amd_shutdown: the set's device is made current, the classes land in a temporary buffer of `count` bytes
 * that is freed on every path, and the download waits for the kernel. */
int eddsa_amd_keyset_classify(const eddsa_amd_keyset *ks, uint8_t *cls)
{
    int saved = -1, rc = 0;
    uint8_t *d_cls = NULL;
    if (!ks || !cls) return -(int)hipErrorInvalidValue;
    if (!edk_point_classify) return -(int)hipErrorNotSupported;
    TRY(hipGetDevice(&saved));
    TRY(hipSetDevice(ks->device));
    TRY(hipMalloc((void **)&d_cls, ks->count));
    TRY(edk_point_classify(d_cls, ks->keys, ks->count, NULL));
    TRY(hipMemcpy(cls, d_cls, ks->count, hipMemcpyDeviceToHost));
out:
    if (d_cls) { HIP_NOTE(hipStreamSynchronize(NULL)); HIP_NOTE(hipFree(d_cls)); }
    if (saved >= 0) HIP_NOTE(hipSetDevice(saved));
    return rc;
}

/* ------------------------------------------------------------------------------------------
 * several devices in one process: contiguous shards, one host thread per device for the
 * host-pointer forms, no data-path collective; the only exchange is the gather of the result bytes
 * (RCCL over xGMI) in the device-pointer form.
 * ---------------------------------------------------------------------------------------- */

void eddsa_amd_shard_bounds(size_t n, int rank, int world, size_t *lo, size_t *hi)
{
    const size_t base = n / (size_t)world, extra = n % (size_t)world, r = (size_t)rank;
    *lo = r * base + (r < extra ? r : extra);
    *hi = *lo + base + (r < extra ? 1 : 0);
}

static int rccl_load(void)
{
    if (!g_multi.rccl) g_multi.rccl = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!g_multi.rccl) g_multi.rccl = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!g_multi.rccl) return ERR_RCCL_MISSING;
#define SYM(field, name) do { *(void **)&g_multi.field = dlsym(g_multi.rccl, name); if (!g_multi.field) return ERR_RCCL_MISSING; } while (0)
    SYM(CommInitAll, "ncclCommInitAll"); SYM(CommDestroy, "ncclCommDestroy"); SYM(AllGather, "ncclAllGather");
    SYM(Broadcast, "ncclBroadcast"); SYM(GroupStart, "ncclGroupStart"); SYM(GroupEnd, "ncclGroupEnd");
    SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
    return 0;
}

int eddsa_amd_init_devices(const int *devices, int n)
{
    int rc = 0, all[MAX_DEVICES];
    if (devices == NULL || n <= 0) {       /* every visible device */
        hipError_t er = hipGetDeviceCount(&n);
        if (er != hipSuccess) return -(int)er;
        if (n > MAX_DEVICES) n = MAX_DEVICES;
        for (int i = 0; i < n; i++) all[i] = i;
        devices = all;
    }
    if (n < 1 || n > MAX_DEVICES) return -(int)hipErrorInvalidValue;
    for (int i = 0; i < n; i++) {
        if (devices[i] < 0 || devices[i] >= MAX_DEVICES) return -(int)hipErrorInvalidDevice;
        for (int k = 0; k < i; k++) if (devices[k] == devices[i]) return -(int)hipErrorInvalidValue;   /* one engine, one RCCL rank per device */
    }
    pthread_rwlock_wrlock(&g_table);
    multi_release();
    for (int i = 0; i < n && !rc; i++) rc = engine_create(devices[i]);
    if (!rc) rc = rccl_load();
    if (!rc) {
        int saved = -1, r;
        HIP_NOTE(hipGetDevice(&saved));
        r = g_multi.CommInitAll(g_multi.comm, n, devices);     /* single process, one communicator per device */
        if (saved >= 0) HIP_NOTE(hipSetDevice(saved));
        if (r) rc = ERR_RCCL_BASE - r;
    }
    if (!rc) {
        g_multi.n = n;
        memcpy(g_multi.dev, devices, (size_t)n * sizeof(int));
        if (g_default < 0) g_default = devices[0];
    } else {
        multi_release();
    }
    pthread_rwlock_unlock(&g_table);
    return rc;
}

int eddsa_amd_device_count(void)
{
    pthread_rwlock_rdlock(&g_table);
    const int n = g_multi.n;
    pthread_rwlock_unlock(&g_table);
    return n;
}

/* the HIP device that owns shard `index` of the set (the order given to eddsa_amd_init_devices), or -1 */
int eddsa_amd_device_at(int index)
{
    pthread_rwlock_rdlock(&g_table);
    const int dev = index >= 0 && index < g_multi.n ? g_multi.dev[index] : -1;
    pthread_rwlock_unlock(&g_table);
    return dev;
}

/* Device-pointer form: device d of the set holds shard d of the inputs and a buffer ok_full[d] of
 * n_total bytes; shard d is verified on device d into its own slice of ok_full[d], then one RCCL
 * all-gather (grouped broadcasts when the shards differ in length) completes every ok_full[d].
 * Everything is enqueued from the calling thread; streams[d] orders the work on device d. */
int ed25519_verify_batch_multi_dev(uint8_t *const ok_full[], const uint8_t *const sigs[], const uint8_t *const pubs[],
                                   const uint8_t *const msgs[], size_t msg_len, size_t n_total, void *const streams[])
{
    int rc = 0, saved = -1, g, r, even = 1, locked = 0;
    void *const no_streams[MAX_DEVICES] = { 0 };
    if (!streams) streams = no_streams;          /* no array: every device's default stream */
    pthread_rwlock_rdlock(&g_table);
    g = g_multi.n;
    if (g == 0) { rc = -(int)hipErrorNotInitialized; goto unlock; }
    if (n_total == 0) goto unlock;
    HIP_NOTE(hipGetDevice(&saved));
    /* concurrent callers must not interleave their launches or their grouped RCCL calls on the shared communicators */
    pthread_mutex_lock(&g_rccl_lk);
    locked = 1;
    for (int d = 0; d < g && !rc; d++) {
        size_t lo, hi;
        eddsa_amd_shard_bounds(n_total, d, g, &lo, &hi);
        if (hi - lo != n_total / (size_t)g) even = 0;
        const struct verify_form plain = { .ks = NULL };
        const edk_verify_src src = verify_src(&plain, sigs[d], pubs[d], msgs[d], NULL, msg_len);
        TRY(hipSetDevice(g_multi.dev[d]));
        rc = verify_on(g_eng[g_multi.dev[d]], ok_full[d] + lo, &src, hi - lo, (hipStream_t)streams[d], NULL, 0);
    }
    if (rc) goto out;
    /* the final result gather: the only exchange of the path */
    if ((r = g_multi.GroupStart())) { rc = ERR_RCCL_BASE - r; goto out; }
    for (int d = 0; d < g; d++) {
        /* a NULL stream is the default stream of the CURRENT device: rank d's calls are made with its device current.
         * (A failure here is reported, but the rank still makes its calls: a group that lacks a rank never completes.) */
        hipError_t er = hipSetDevice(g_multi.dev[d]);
        if (er != hipSuccess && !rc) rc = -(int)er;
        if (even) {
            size_t lo, hi;
            eddsa_amd_shard_bounds(n_total, d, g, &lo, &hi);
            r = g_multi.AllGather(ok_full[d] + lo, ok_full[d], hi - lo, NCCL_UINT8, g_multi.comm[d], (hipStream_t)streams[d]);
            if (r && !rc) rc = ERR_RCCL_BASE - r;
        } else {
            for (int root = 0; root < g; root++) {
                size_t lo, hi;
                eddsa_amd_shard_bounds(n_total, root, g, &lo, &hi);
                r = g_multi.Broadcast(ok_full[d] + lo, ok_full[d] + lo, hi - lo, NCCL_UINT8, root, g_multi.comm[d],
                                      (hipStream_t)streams[d]);
                if (r && !rc) rc = ERR_RCCL_BASE - r;
            }
        }
    }
    r = g_multi.GroupEnd();
    if (r && !rc) rc = ERR_RCCL_BASE - r;
out:
    if (locked) pthread_mutex_unlock(&g_rccl_lk);
    if (saved >= 0) HIP_NOTE(hipSetDevice(saved));
unlock:
    pthread_rwlock_unlock(&g_table);
    return rc;
}

/* ------------------------------------------------------------------------------------------
 * diagnostics
 * ---------------------------------------------------------------------------------------- */

int count_nonzero_dev(const void *dev, size_t bytes, uint64_t *count)
{
    int rc = 0;
    if (!dev || !bytes) return 0;
    uint8_t *h = (uint8_t *)malloc(bytes);
    if (!h) return -(int)hipErrorOutOfMemory;
    TRY(hipMemcpy(h, dev, bytes, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < bytes; i++) *count += h[i] != 0;
out:
    free(h);
    return rc;
}

/* ------------------------------------------------------------------------------------------
 * the test and measurement surface (include/eddsa_amd_debug.h): only libeddsa_amd_debug.so has it; the fault injectors
 * are inert unless armed
 * ---------------------------------------------------------------------------------------- */

#ifdef EDDSA_AMD_DEBUG_BUILD
int eddsa_amd_debug_init(int device, unsigned flags)
{
    const int rc = eddsa_amd_init(device);
    if (rc) return rc;
    __atomic_store_n(&g_hooks_armed, (flags & EDDSA_AMD_TEST_HOOKS) != 0, __ATOMIC_RELEASE);
    edk_debug_counting((flags & EDDSA_AMD_TEST_HOOKS) != 0);
    if (!(flags & EDDSA_AMD_TEST_HOOKS)) (void)edk_debug_fail_in(0);
    return 0;
}

int eddsa_amd_debug_fail_hip_call(int nth)
{
    if (!__atomic_load_n(&g_hooks_armed, __ATOMIC_ACQUIRE)) return EDDSA_AMD_HOOKS_OFF;
    (void)edk_debug_fail_in(nth < 0 ? 0 : nth);
    return 0;
}

int eddsa_amd_debug_hip_calls(void)
{
    return edk_debug_fail_in(-1);
}

int eddsa_amd_debug_withhold_handoff(int tile_plus_1)
{
    struct call c;
    int rc, gave_up = 0;
    if (!__atomic_load_n(&g_hooks_armed, __ATOMIC_ACQUIRE)) return EDDSA_AMD_HOOKS_OFF;
    if ((rc = enter(&c, -1))) return rc;
    pthread_mutex_lock(&c.e->lk);
    TRY(hipDeviceSynchronize());
    for (int i = 0; i < VERIFY_SLOTS; i++) {
        const uint32_t w = tile_plus_1 > 0 ? (uint32_t)tile_plus_1 : 0u;
        if (c.e->vs[i].ws.offcount) TRY(hipMemcpy(c.e->vs[i].ws.offcount + EDK_WITHHOLD_WORD, &w, sizeof(w), hipMemcpyHostToDevice));
        if (c.e->vs[i].rws.base) {
            uint32_t *hook = (uint32_t *)((char *)c.e->vs[i].rws.base + edk_rlc_hook_offset(c.e->vs[i].rws.capacity));
            uint32_t two[2] = { 0, 0 };
            TRY(hipMemcpy(two, hook, sizeof(two), hipMemcpyDeviceToHost));
            gave_up += (int)two[1];
            two[0] = w; two[1] = 0;
            TRY(hipMemcpy(hook, two, sizeof(two), hipMemcpyHostToDevice));
        }
    }
    rc = gave_up;
out:
    pthread_mutex_unlock(&c.e->lk);
    leave(&c);
    return rc;
}

int eddsa_amd_dump_tables(uint32_t *base16_words, uint32_t *comb_words)
{
    struct call c;
    int rc = enter(&c, -1);
    if (rc) return rc;
    TRY(hipMemcpy(base16_words, c.e->base16, (size_t)TABLE_BASE16_ENTRIES * TABLE_ENTRY_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost));
    TRY(hipMemcpy(comb_words, c.e->comb, TABLE_COMB_ENTRIES * TABLE_ENTRY_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost));
out:
    leave(&c);
    return rc;
}

/* one key's comb of a comb key set, for the tests that hold it against integers: reads only, on the key set's device */
int eddsa_amd_debug_keyset_comb_read(const eddsa_amd_keyset *ks, size_t key, uint32_t *words)
{
    struct call c;
    int rc;
    if (!ks || !ks->comb || !words || key >= ks->count) return -(int)hipErrorInvalidValue;
    if ((rc = enter(&c, ks->device))) return rc;
    TRY(hipMemcpy(words, ks->comb + key * KEYSET_COMB_WORDS, KEYSET_COMB_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost));
out:
    leave(&c);
    return rc;
}

/* One region of what the last pass of the batch verification on the default device left in its workspace (include/eddsa_amd_debug.h;
 * the layout is rlc.hip's: edk_rlc_region).  Reads only, after the device has gone idle.
 * edk_rlc_region is a WEAK reference: the host side is also linked without rlc.hip (tests/fake_hip, whose launchers decide every item
 * one by one: there is no combination to take a snapshot of, and that build stands in for none of it) - the call is then
 * hipErrorNotSupported. */
extern __typeof__(edk_rlc_region) edk_rlc_region __attribute__((weak));
int eddsa_amd_debug_rlc_snapshot(int region, void *out, size_t out_bytes)
{
    struct call c;
    int rc;
    if (!edk_rlc_region) return -(int)hipErrorNotSupported;
    if ((rc = enter(&c, -1))) return rc;
    pthread_mutex_lock(&c.e->lk);
    const struct vslot *v = &c.e->vs[c.e->snap_slot];
    const size_t n = c.e->snap_n;
    edk_rlc_span s;
    TRY(hipDeviceSynchronize());
    if (n == 0 || !v->rws.base) { rc = -(int)hipErrorNotReady; goto out; }
    if (region == EDDSA_AMD_RLC_INFO) {
        if (!out || out_bytes < 3 * sizeof(uint64_t) || !edk_rlc_region(&s, EDDSA_AMD_RLC_GOK, v->rws.capacity, n)) { rc = -(int)hipErrorInvalidValue; goto out; }
        const uint64_t info[3] = { n, s.bytes, v->rws.capacity };   /* (one verdict byte per group) */
        memcpy(out, info, sizeof(info));
        rc = (int)sizeof(info);
        goto out;
    }
    if (!out || !edk_rlc_region(&s, region, v->rws.capacity, n) || out_bytes < s.bytes * s.count) { rc = -(int)hipErrorInvalidValue; goto out; }
    for (size_t k = 0; k < s.count; k++)
        TRY(hipMemcpy((char *)out + k * s.bytes, (const char *)v->rws.base + s.offset + k * s.stride, s.bytes, hipMemcpyDeviceToHost));
    rc = (int)(s.bytes * s.count);
out:
    pthread_mutex_unlock(&c.e->lk);
    leave(&c);
    return rc;
}

/* Which evaluation ed25519_verify* uses (same verdicts; a measurement and test aid).  0 (default): half-length
 * scalars (csrc/halve.h), four lanes per item up to 2^15 items and one above; 1: full-length windows always;
 * 2: half-length scalars with one lane per item always; 3: the mid-size arrangement below 2^18 items; 4: the arrangement of
 * full-size passes (balanced pairs, 33 windows) at any size.  Any other value: 0. */
void eddsa_amd_set_verify_algo(int algo)
{
    pthread_rwlock_wrlock(&g_table);
    g_verify_algo = algo >= 1 && algo <= 4 ? algo : 0;
    pthread_rwlock_unlock(&g_table);
}

/* diagnostic for the tests: how many half-length pairs the exact integer check (csrc/lanes.h: verify_half_scalars_lane)
 * has refused on the default device since its workspaces were allocated.  Waits for the device.  Expected: 0. */
int eddsa_amd_halve_rejected(uint64_t *count)
{
    struct call c;
    int rc = enter(&c, -1);
    if (rc) return rc;
    *count = 0;
    pthread_mutex_lock(&c.e->lk);
    TRY(hipDeviceSynchronize());
    for (int i = 0; i < VERIFY_SLOTS; i++) {
        uint32_t w = 0;
        if (!c.e->vs[i].ws.offcount) continue;
        TRY(hipMemcpy(&w, c.e->vs[i].ws.offcount + EDK_REFUSED_WORD, sizeof(w), hipMemcpyDeviceToHost));
        *count += w;
    }
out:
    pthread_mutex_unlock(&c.e->lk);
    leave(&c);
    return rc;
}

int eddsa_amd_debug_teardown_errors(int *first_hip_error)
{
    if (first_hip_error) *first_hip_error = __atomic_load_n(&g_teardown.first, __ATOMIC_ACQUIRE);
    return __atomic_load_n(&g_teardown.count, __ATOMIC_ACQUIRE);
}

/* per-kernel timing of the verify pass, for bench.py's roofline line: HIP events recorded on the
 * launch stream around k_verify_prepare / k_verify_main / k_verify_finish of every chunk */
void eddsa_amd_set_profiling(int on)
{
    pthread_rwlock_wrlock(&g_table);       /* no call in flight: nobody is bumping marks_used */
    g_profiling = on != 0;
    for (int d = 0; d < MAX_DEVICES; d++) if (g_eng[d]) g_eng[d]->marks_used = 0;
    pthread_rwlock_unlock(&g_table);
}

/* average duration (ms) of each of the three kernels over the passes recorded on the default device
 * since profiling was switched on (at most MARK_SLOTS; later passes are not recorded) */
int eddsa_amd_verify_phase_ms(float out[3])
{
    struct call c;
    int rc = enter(&c, -1);
    if (rc) return rc;
    pthread_mutex_lock(&c.e->lk);
    const int used = c.e->marks_used < MARK_SLOTS ? c.e->marks_used : MARK_SLOTS;
    if (used == 0) { rc = -(int)hipErrorNotReady; goto out; }
    out[0] = out[1] = out[2] = 0.0f;
    for (int s = 0; s < used; s++) {
        TRY(hipEventSynchronize(c.e->marks[s][3]));
        for (int i = 0; i < 3; i++) {
            float ms = 0.0f;
            TRY(hipEventElapsedTime(&ms, c.e->marks[s][i], c.e->marks[s][i + 1]));
            out[i] += ms / (float)used;
        }
    }
out:
    pthread_mutex_unlock(&c.e->lk);
    leave(&c);
    return rc;
}

/* Secret hygiene check (tests): non-zero bytes left on the default device in out[0] the scalar
 * workspace `aux` (sign's a and r), out[1] the point workspace `acc` (x25519's (x2 : z2); public for
 * the other operations), out[2] the host pipeline's first input staging buffers (secret keys /
 * scalars), out[3] its output staging buffer.  Waits for the device to go idle first. */
int eddsa_amd_secret_residue(uint64_t out[4])
{
    struct call c;
    int rc = enter(&c, -1);
    if (rc) return rc;
    out[0] = out[1] = out[2] = out[3] = 0;
    pthread_mutex_lock(&c.e->lk);
    TRY(hipDeviceSynchronize());
    for (int i = 0; i < VERIFY_SLOTS && !rc; i++) {
        const struct vslot *v = &c.e->vs[i];
        rc = count_nonzero_dev(v->fws.aux, fws_aux_bytes(v->fws.capacity), &out[0]);
        if (!rc) rc = count_nonzero_dev(v->fws.acc, fws_acc_bytes(v->fws.capacity), &out[1]);
    }
out:
    pthread_mutex_unlock(&c.e->lk);
    if (!rc) rc = pipe_residue(c.e, &out[2], &out[3]);
    leave(&c);
    return rc;
}
#endif
