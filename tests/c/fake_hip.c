/* A recording stand-in for the HIP runtime, for running the HOST side of liblcs_hip under AddressSanitizer / UBSan on a
 * machine without a GPU (tests/test_host_orchestration_asan.py).
 *
 * "Device" memory is host memory from malloc (so a buffer overrun of a copy, a use after free, a double free or a leak is
 * the sanitizer's to report), copies are memcpy / memset, kernel launches are counted and do nothing (outputs are
 * whatever the buffers held: the tests look at status codes and at what was allocated and freed, not at numbers),
 * streams are opaque tokens.  hipMalloc / hipMallocAsync fail with hipErrorOutOfMemory at the call number
 * fake_hip_fail_malloc_at() names, and any copy at fake_hip_fail_memcpy_at(): every early-return path of the host routes
 * is then walked once.  Callable from several threads at once, as the real runtime is (the books behind one lock, the last error
 * and the pushed launch configuration per thread).  Only what csrc/ *.hip call is here; a new call shows up as an undefined symbol at link time.
 *
 * An optional TRACE (off unless fake_hip_trace_begin() is called; tests/c/host_route_trace.cpp): every launch with the kernel's
 * registered name, grid, block and stream, every copy and memset with kind, bytes, destination and source, every event record,
 * stream wait and synchronise, one line each as it happens, and at fake_hip_trace_end() the sizes of the allocations made in
 * between, sorted.  Nothing in a trace is an address: a device or pinned buffer is "the n-th distinct buffer in order of first
 * use" + offset (dev<n>+off, pin<n>+off), a stream or event likewise (s<n>, e<n>), a host pointer inside an array the caller
 * named with fake_hip_trace_host() is name+offset and any other is "local" -- so a trace does not depend on where malloc put
 * things, nor on the order of a call's allocations alone. */
#include <hip/hip_runtime_api.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define MAX_LIVE 4096
static void *g_live[MAX_LIVE];
static size_t g_live_bytes[MAX_LIVE];
static int g_nlive, g_mallocs, g_frees, g_launches, g_copies, g_fail_malloc_at, g_fail_memcpy_at, g_bad_free;
static char g_live_pinned[MAX_LIVE];
static _Thread_local hipError_t g_last = hipSuccess;
static pthread_mutex_t g_books = PTHREAD_MUTEX_INITIALIZER;
#define LOCKED(stmt) do { pthread_mutex_lock(&g_books); stmt; pthread_mutex_unlock(&g_books); } while (0)

/* ---- the trace (all of it behind g_books) ---- */
#define MAX_IDS 512
static FILE *g_trace;                                   /* NULL: off */
static struct { const void *p; char kind; int id; } g_ids[MAX_IDS];   /* kind: 'd'evice, 'p'inned, 's'tream, 'e'vent */
static int g_nids, g_next_id[128];
static struct { const char *name; const char *base; size_t bytes; } g_hosts[16];
static int g_nhosts;
static size_t *g_trace_allocs;
static int g_ntrace_allocs, g_cap_trace_allocs;
static struct { const void *host; const char *name; } *g_kernels;       /* what __hipRegisterFunction was told, always kept */
static int g_nkernels, g_cap_kernels;

static int trace_id(const void *p, char kind) {        /* n-th distinct object of its kind in order of first use */
    for (int i = 0; i < g_nids; ++i)
        if (g_ids[i].p == p && g_ids[i].kind == kind) return g_ids[i].id;
    if (g_nids == MAX_IDS) { fprintf(stderr, "fake_hip: trace id table full\n"); abort(); }
    g_ids[g_nids].p = p; g_ids[g_nids].kind = kind;
    return g_ids[g_nids++].id = g_next_id[(int)kind]++;
}
static void trace_forget(const void *p) {               /* freed: the address may come back as another object */
    for (int i = 0; i < g_nids; ++i)
        if (g_ids[i].p == p) g_ids[i--] = g_ids[--g_nids];
}
static const char *trace_ptr(const void *p, char *buf, size_t n) {
    if (!p) return "null";
    for (int i = 0; i < g_nhosts; ++i)
        if ((const char *)p >= g_hosts[i].base && (const char *)p < g_hosts[i].base + g_hosts[i].bytes) {
            snprintf(buf, n, "%s+%zu", g_hosts[i].name, (size_t)((const char *)p - g_hosts[i].base));
            return buf;
        }
    for (int i = 0; i < g_nlive; ++i)
        if ((const char *)p >= (const char *)g_live[i] && (const char *)p < (const char *)g_live[i] + (g_live_bytes[i] ? g_live_bytes[i] : 1)) {
            snprintf(buf, n, "%s%d+%zu", g_live_pinned[i] ? "pin" : "dev", trace_id(g_live[i], g_live_pinned[i] ? 'p' : 'd'),
                     (size_t)((const char *)p - (const char *)g_live[i]));
            return buf;
        }
    return "local";
}
static const char *trace_stream(hipStream_t s, char *buf, size_t n) {
    if (!s) return "s-null";
    snprintf(buf, n, "s%d", trace_id(s, 's'));
    return buf;
}
#define TRACE(...) do { if (g_trace) { pthread_mutex_lock(&g_books); if (g_trace) { __VA_ARGS__; } pthread_mutex_unlock(&g_books); } } while (0)
static void trace_copy(const char *call, void *d, const void *s, size_t n, hipMemcpyKind k, hipStream_t st, int with_stream) {
    static const char *const kinds[] = {"H2H", "H2D", "D2H", "D2D", "default"};
    char a[64], b[64], c[32];
    const char *dst = trace_ptr(d, a, sizeof a), *src = trace_ptr(s, b, sizeof b);   /* (ids are given in this order: one statement each) */
    const char *on = with_stream ? trace_stream(st, c, sizeof c) : "-";
    fprintf(g_trace, "%s %s %zu %s <- %s on %s\n", call, (unsigned)k < 5 ? kinds[k] : "?", n, dst, src, on);
}
void fake_hip_trace_host(const char *name, const void *base, size_t bytes) {   /* an array of the caller's, by name (16 at most; before trace_begin) */
    pthread_mutex_lock(&g_books);
    if (g_nhosts == 16) { fprintf(stderr, "fake_hip: too many named host arrays\n"); abort(); }
    g_hosts[g_nhosts].name = name; g_hosts[g_nhosts].base = (const char *)base; g_hosts[g_nhosts++].bytes = bytes;
    pthread_mutex_unlock(&g_books);
}
void fake_hip_trace_begin(FILE *out) {
    pthread_mutex_lock(&g_books);
    g_trace = out; g_nids = 0; g_ntrace_allocs = 0;
    memset(g_next_id, 0, sizeof g_next_id);
    pthread_mutex_unlock(&g_books);
}
static int cmp_size(const void *a, const void *b) { size_t x = *(const size_t *)a, y = *(const size_t *)b; return x < y ? -1 : x > y; }
void fake_hip_trace_end(void) {                         /* the allocations since trace_begin, sorted; forgets the named host arrays */
    pthread_mutex_lock(&g_books);
    if (g_trace) {
        if (g_ntrace_allocs) qsort(g_trace_allocs, (size_t)g_ntrace_allocs, sizeof(size_t), cmp_size);   /* (never allocated: NULL) */
        fprintf(g_trace, "allocs");
        for (int i = 0; i < g_ntrace_allocs; ++i) fprintf(g_trace, " %zu", g_trace_allocs[i]);
        fprintf(g_trace, "\n");
    }
    g_trace = NULL; g_nhosts = 0;
    pthread_mutex_unlock(&g_books);
}
static void trace_alloc(size_t bytes) {                 /* (g_books held) */
    if (!g_trace) return;
    if (g_ntrace_allocs == g_cap_trace_allocs) {
        g_cap_trace_allocs = g_cap_trace_allocs ? 2 * g_cap_trace_allocs : 64;
        g_trace_allocs = (size_t *)realloc(g_trace_allocs, (size_t)g_cap_trace_allocs * sizeof(size_t));
        if (!g_trace_allocs) abort();
    }
    g_trace_allocs[g_ntrace_allocs++] = bytes;
}

int fake_hip_live(void) { int n; LOCKED(n = g_nlive); return n; }
int fake_hip_mallocs(void) { return g_mallocs; }
int fake_hip_frees(void) { return g_frees; }
int fake_hip_launches(void) { return g_launches; }
int fake_hip_copies(void) { return g_copies; }
int fake_hip_bad_frees(void) { return g_bad_free; }
void fake_hip_fail_malloc_at(int n) { g_fail_malloc_at = n; }   /* the n-th allocation from now (1 = the next) fails; 0 = never */
void fake_hip_fail_memcpy_at(int n) { g_fail_memcpy_at = n; }
void fake_hip_reset_counts(void) { g_mallocs = g_frees = g_launches = g_copies = 0; }

static hipError_t do_malloc(void **p, size_t bytes, int pinned) {
    int refuse;
    LOCKED(++g_mallocs; refuse = (g_fail_malloc_at > 0 && --g_fail_malloc_at == 0) || g_nlive == MAX_LIVE);
    *p = refuse ? NULL : malloc(bytes ? bytes : 1);
    if (!*p) return g_last = hipErrorOutOfMemory;
    LOCKED(g_live[g_nlive] = *p; g_live_pinned[g_nlive] = (char)pinned; g_live_bytes[g_nlive++] = bytes; if (!pinned) trace_alloc(bytes));
    return hipSuccess;
}
static hipError_t do_free(void *p) {
    if (!p) return hipSuccess;
    int found = 0;
    pthread_mutex_lock(&g_books);
    for (int i = 0; i < g_nlive && !found; ++i)
        if (g_live[i] == p) {
            g_live[i] = g_live[--g_nlive];
            g_live_bytes[i] = g_live_bytes[g_nlive];
            g_live_pinned[i] = g_live_pinned[g_nlive];
            trace_forget(p);
            ++g_frees;
            found = 1;
        }
    if (!found) ++g_bad_free; /* not ours, or freed twice */
    pthread_mutex_unlock(&g_books);
    if (!found) return g_last = hipErrorInvalidValue;
    free(p);
    return hipSuccess;
}
static hipError_t do_copy(void *dst, const void *src, size_t n) {
    int refuse;
    LOCKED(++g_copies; refuse = g_fail_memcpy_at > 0 && --g_fail_memcpy_at == 0);
    if (refuse) return g_last = hipErrorInvalidValue;
    if (n) memcpy(dst, src, n); /* an overrun of either side is ASan's to catch */
    return hipSuccess;
}

hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t a, int d) { (void)a; (void)d; *v = 256; return hipSuccess; }
hipError_t hipSetDevice(int d) { return d == 0 ? hipSuccess : (g_last = hipErrorInvalidDevice); }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags) { (void)flags; *s = (hipStream_t)malloc(1); return *s ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipStreamDestroy(hipStream_t s) { LOCKED(trace_forget(s)); free(s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) {
    char a[32];
    TRACE(fprintf(g_trace, "stream_sync %s\n", trace_stream(s, a, sizeof a)));
    return hipSuccess;
}
/* pinned host memory, events, cross-stream waits (the host routes' staging ring, csrc/hostxfer.h): host memory is host memory here,
 * every "asynchronous" operation has completed when its call returns, so events are tokens and waits are no-ops.  Pinned
 * allocations are counted like device ones (a leak of either shows in fake_hip_live()). */
static int g_fail_host_malloc = 0;
void fake_hip_fail_host_malloc(int on) { g_fail_host_malloc = on; }    /* 1: hipHostMalloc fails (the routes must fall back to plain copies) */
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned flags) {
    (void)flags;
    if (g_fail_host_malloc) { *p = NULL; return g_last = hipErrorOutOfMemory; }
    return do_malloc(p, bytes, 1);
}
hipError_t hipHostFree(void *p) { return do_free(p); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags) { (void)flags; *e = (hipEvent_t)malloc(1); return *e ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipEventDestroy(hipEvent_t e) { LOCKED(trace_forget(e)); free(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    char a[32];
    TRACE(const int id = trace_id(e, 'e'); fprintf(g_trace, "event_record e%d on %s\n", id, trace_stream(s, a, sizeof a)));
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) {
    TRACE(fprintf(g_trace, "event_sync e%d\n", trace_id(e, 'e')));
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags) {
    char a[32];
    (void)flags;
    TRACE(const char *on = trace_stream(s, a, sizeof a); fprintf(g_trace, "stream_wait %s for e%d\n", on, trace_id(e, 'e')));
    return hipSuccess;
}
hipError_t hipMalloc(void **p, size_t bytes) { return do_malloc(p, bytes, 0); }
hipError_t hipMallocAsync(void **p, size_t bytes, hipStream_t s) { (void)s; return do_malloc(p, bytes, 0); }
hipError_t hipFree(void *p) { return do_free(p); }
hipError_t hipFreeAsync(void *p, hipStream_t s) { (void)s; return do_free(p); }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind k) {
    TRACE(trace_copy("memcpy", d, s, n, k, NULL, 0));
    return do_copy(d, s, n);
}
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind k, hipStream_t st) {
    TRACE(trace_copy("memcpy_async", d, s, n, k, st, 1));
    return do_copy(d, s, n);
}
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t st) {
    char a[64], b[32];
    TRACE(const char *dst = trace_ptr(d, a, sizeof a); fprintf(g_trace, "memset_async %d %zu %s on %s\n", v, n, dst, trace_stream(st, b, sizeof b)));
    memset(d, v, n);
    return hipSuccess;
}
hipError_t hipGetLastError(void) { hipError_t e = g_last; g_last = hipSuccess; return e; }
const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : (e == hipErrorOutOfMemory ? "out of memory (injected)" : "fake HIP error"); }
hipError_t hipLaunchKernel(const void *f, dim3 grid, dim3 block, void **args, size_t shmem, hipStream_t st) {
    (void)args;
    pthread_mutex_lock(&g_books);
    ++g_launches;
    if (g_trace) {
        const char *name = "?";
        char a[32];
        for (int i = 0; i < g_nkernels; ++i)
            if (g_kernels[i].host == f) { name = g_kernels[i].name; break; }
        fprintf(g_trace, "launch %s grid %u,%u,%u block %u,%u,%u lds %zu on %s\n", name, grid.x, grid.y, grid.z, block.x, block.y, block.z, shmem,
                trace_stream(st, a, sizeof a));
    }
    pthread_mutex_unlock(&g_books);
    if (grid.x == 0 || grid.y == 0 || grid.z == 0 || block.x * block.y * block.z == 0 || block.x * block.y * block.z > 1024 || grid.y > 65535 || grid.z > 65535)
        return g_last = hipErrorInvalidConfiguration; /* what the real runtime refuses */
    return hipSuccess;
}
/* what hipcc's host stubs call */
static _Thread_local struct { dim3 grid, block; size_t shmem; hipStream_t st; } g_cfg;
void **__hipRegisterFatBinary(const void *data) { (void)data; static void *h; return &h; }
void __hipUnregisterFatBinary(void **h) { (void)h; }
void __hipRegisterFunction(void **h, const void *host, char *dev, const char *name, int tl, void *a, void *b, void *c, void *d, int *e) {
    (void)h; (void)dev; (void)tl; (void)a; (void)b; (void)c; (void)d; (void)e;
    pthread_mutex_lock(&g_books);        /* (kept for the life of the process: a few thousand pointers) */
    if (g_nkernels == g_cap_kernels) {
        g_cap_kernels = g_cap_kernels ? 2 * g_cap_kernels : 1024;
        g_kernels = realloc(g_kernels, (size_t)g_cap_kernels * sizeof *g_kernels);
        if (!g_kernels) abort();
    }
    g_kernels[g_nkernels].host = host; g_kernels[g_nkernels++].name = name;
    pthread_mutex_unlock(&g_books);
}
void __hipRegisterVar(void **h, void *var, char *a, char *b, int ext, size_t size, int constant, int global) {
    (void)h; (void)var; (void)a; (void)b; (void)ext; (void)size; (void)constant; (void)global;
}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t st) {
    g_cfg.grid = grid; g_cfg.block = block; g_cfg.shmem = shmem; g_cfg.st = st;
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3 *grid, dim3 *block, size_t *shmem, hipStream_t *st) {
    *grid = g_cfg.grid; *block = g_cfg.block; *shmem = g_cfg.shmem; *st = g_cfg.st;
    return hipSuccess;
}
