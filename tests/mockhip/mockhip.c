// tests/mockhip/mockhip.c -- TEST INFRASTRUCTURE, not a CPU path of the product: a stand-in for the HIP runtime whose kernels do
// NOTHING (hipLaunchKernel returns at once, device memory is zeroed host memory), preloaded by tests/test_planner_host.py so that
// the HOST side of the library -- segment bookkeeping, the planner, the result unpacking -- can be executed on a box without a GPU.
// Every search under it returns empty results; what is learned is that the host code runs through and what plan it builds
// (NRTGPU_PLAN_TRACE).  The product never loads this: nrtgpu_create fails without a gfx950 device (tests/test_abi.py).
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <stdio.h>
#include <pthread.h>
#include <stdint.h>
static long n_launch = 0;
// MOCKHIP_TRACE_OPS=1 (with MOCKHIP_TRACE; off: the trace holds kernel launches only, as before): one line per copy, asynchronous
// memset, event record, stream wait and synchronisation as well.  A pointer is printed as its offset inside the hipMalloc (`d+`) or
// hipHostMalloc (`h+`) allocation that contains it, `ext` when the mock allocated none; an event as the ordinal of its creation.
// No absolute address appears, so two runs of one script write the same file.
static int trace_ops = 0;
static FILE* trace_out = NULL;
static pthread_mutex_t alloc_mu = PTHREAD_MUTEX_INITIALIZER;
static struct { const char* p; size_t n; char kind; } allocs[1 << 16];
static int n_allocs = 0;
static void alloc_note(void* p, size_t n, char kind) {
  if (!trace_ops) return;
  pthread_mutex_lock(&alloc_mu);
  if (n_allocs < (1 << 16)) { allocs[n_allocs].p = (const char*)p; allocs[n_allocs].n = n ? n : 1; allocs[n_allocs].kind = kind; ++n_allocs; }
  pthread_mutex_unlock(&alloc_mu);
}
static void alloc_forget(void* p) {
  if (!trace_ops || !p) return;
  pthread_mutex_lock(&alloc_mu);
  for (int i = 0; i < n_allocs; ++i) if (allocs[i].p == (const char*)p) { allocs[i] = allocs[--n_allocs]; break; }
  pthread_mutex_unlock(&alloc_mu);
}
static const char* where(const void* p, char* buf) {
  strcpy(buf, "ext");
  pthread_mutex_lock(&alloc_mu);
  for (int i = 0; i < n_allocs; ++i)
    if ((const char*)p >= allocs[i].p && (const char*)p < allocs[i].p + allocs[i].n) { sprintf(buf, "%c+%zu", allocs[i].kind, (size_t)((const char*)p - allocs[i].p)); break; }
  pthread_mutex_unlock(&alloc_mu);
  return buf;
}
static void trace_copy(const char* what, void* d, const void* s, size_t n, hipMemcpyKind k) {
  if (!trace_ops || !trace_out) return;
  static const char* kinds[] = {"H2H", "H2D", "D2H", "D2D", "default"};
  char bd[32], bs[32];
  fprintf(trace_out, "%s %s %zu dst=%s src=%s\n", what, kinds[(unsigned)k < 5 ? (unsigned)k : 4], n, where(d, bd), where(s, bs));
  fflush(trace_out);
}
static void trace_event(const char* what, hipEvent_t e) {
  if (!trace_ops || !trace_out) return;
  if (e) fprintf(trace_out, "%s e%ld\n", what, *(const long*)e);
  else fprintf(trace_out, "%s\n", what);
  fflush(trace_out);
}
static hipEvent_t new_event(void) {
  static long n_events = 0;
  long* e = (long*)malloc(8);
  *e = __atomic_add_fetch(&n_events, 1, __ATOMIC_SEQ_CST);
  return (hipEvent_t)e;
}
hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int d) { (void)d; return hipSuccess; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_t* p, int d) {
  (void)d; memset(p, 0, sizeof *p); p->multiProcessorCount = 256; strcpy(p->gcnArchName, "gfx950:sramecc+:xnack-");
  p->totalGlobalMem = (size_t)288 << 30; p->sharedMemPerBlock = 160 * 1024; p->warpSize = 64; p->maxThreadsPerBlock = 1024; return hipSuccess; }
static hipError_t mock_alloc(void** p, size_t n, char kind) {
  void* q = NULL; if (posix_memalign(&q, 256, n ? n : 256)) return hipErrorOutOfMemory; memset(q, 0, n); alloc_note(q, n, kind); *p = q; return hipSuccess; }
hipError_t hipMalloc(void** p, size_t n) { return mock_alloc(p, n, 'd'); }
hipError_t hipFree(void* p) { alloc_forget(p); free(p); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned f) { (void)f; return mock_alloc(p, n, 'h'); }
hipError_t hipHostFree(void* p) { alloc_forget(p); free(p); return hipSuccess; }
hipError_t hipHostRegister(void* p, size_t n, unsigned f) { (void)p; (void)n; (void)f; return hipSuccess; }
hipError_t hipHostUnregister(void* p) { (void)p; return hipSuccess; }
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned f) { (void)f; *d = h; return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind k) { trace_copy("memcpy", d, s, n, k); if (n) memmove(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind k, hipStream_t st) { (void)st; trace_copy("memcpyAsync", d, s, n, k); if (n) memmove(d, s, n); return hipSuccess; }
hipError_t hipMemcpy2D(void* d, size_t dp, const void* s, size_t sp, size_t w, size_t h, hipMemcpyKind k) {
  (void)k; for (size_t r = 0; r < h; ++r) memmove((char*)d + r * dp, (const char*)s + r * sp, w); return hipSuccess; }
hipError_t hipMemset(void* d, int v, size_t n) { memset(d, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t st) {
  (void)st;
  if (trace_ops && trace_out) { char b[32]; fprintf(trace_out, "memsetAsync %s %d %zu\n", where(d, b), v, n); fflush(trace_out); }
  memset(d, v, n); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned f) { (void)f; *s = (hipStream_t)malloc(8); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { free(s); return hipSuccess; }
/* MOCKHIP_SYNC_US: how long a stream synchronisation "takes" (0 by default): lets a test keep searches in flight for a while */
static void mock_sync_delay(void) {
  static int us = -1;
  if (us < 0) { const char* e = getenv("MOCKHIP_SYNC_US"); us = e ? atoi(e) : 0; }
  if (us > 0) usleep((useconds_t)us);
}
hipError_t hipStreamSynchronize(hipStream_t s) { (void)s; trace_event("streamSynchronize", NULL); mock_sync_delay(); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned f) { (void)s; (void)f; trace_event("streamWaitEvent", e); return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { *e = new_event(); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned f) { (void)f; *e = new_event(); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { free(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { (void)s; trace_event("eventRecord", e); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { trace_event("eventSynchronize", e); return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) { (void)a; (void)b; *ms = 0.001f; return hipSuccess; }
// mockhip_fail_next_launches(n): the next n kernel launches fail (hipErrorLaunchFailure, also what the launching thread's next
// hipGetLastError() says, once): how a test sees what the library does with a launch that failed
static int fail_launches = 0;
static __thread hipError_t sticky_error = hipSuccess;
void mockhip_fail_next_launches(int n) { __atomic_store_n(&fail_launches, n, __ATOMIC_SEQ_CST); }
hipError_t hipGetLastError(void) { hipError_t e = sticky_error; sticky_error = hipSuccess; return e; }
const char* hipGetErrorString(hipError_t e) { (void)e; return "mock hip"; }
hipError_t hipFuncSetAttribute(const void* f, hipFuncAttribute a, int v) { (void)f; (void)a; (void)v; return hipSuccess; }
// MOCKHIP_TRACE=<file>: one line per hipLaunchKernel -- the device kernel's name (remembered from __hipRegisterFunction), grid.x,
// block.x, dynamic shared bytes -- so that a test can compare the launch schedule of two builds of the library
static struct { const void* host; const char* name; } kernels[1024];
static int n_kernels = 0;
__attribute__((constructor)) static void trace_open(void) {   // (before any thread of the program exists)
  const char* e = getenv("MOCKHIP_TRACE");
  if (e && *e) trace_out = fopen(e, "w");
  const char* o = getenv("MOCKHIP_TRACE_OPS");
  trace_ops = trace_out && o && *o && strcmp(o, "0") != 0;
}
// mockhip_poke_arg(name, arg, elem, value, times): on the next `times` launches of a kernel whose name contains `name`, store
// `value` as the uint64 number `elem` of the array that the launch's pointer argument number `arg` points at -- the one thing a
// kernel that does nothing cannot do for a test: leave a word in its output (a tag in a hit total, say) for the host code to act on.
// Several pokes may be pending at once.
static struct { char name[64]; int arg; long elem; uint64_t value; int times; } pokes[256];
static int n_pokes = 0;
static pthread_mutex_t poke_mu = PTHREAD_MUTEX_INITIALIZER;
void mockhip_poke_arg(const char* name, int arg, long elem, uint64_t value, int times) {
  pthread_mutex_lock(&poke_mu);
  if (n_pokes < 256 && times > 0) {
    strncpy(pokes[n_pokes].name, name, 63); pokes[n_pokes].name[63] = 0;
    pokes[n_pokes].arg = arg; pokes[n_pokes].elem = elem; pokes[n_pokes].value = value; pokes[n_pokes].times = times; ++n_pokes;
  }
  pthread_mutex_unlock(&poke_mu);
}
static void poke_launch(const char* name, void** args) {
  if (!n_pokes) return;
  pthread_mutex_lock(&poke_mu);
  for (int i = 0; i < n_pokes;) {
    if (strstr(name, pokes[i].name)) {
      (*(uint64_t**)args[pokes[i].arg])[pokes[i].elem] = pokes[i].value;
      if (--pokes[i].times == 0) { pokes[i] = pokes[--n_pokes]; continue; }
    }
    ++i;
  }
  pthread_mutex_unlock(&poke_mu);
}
static const char* kernel_name(const void* f) {
  for (int i = 0; i < n_kernels; ++i) if (kernels[i].host == f) return kernels[i].name;
  return "?";
}
static void trace_launch(const void* f, dim3 g, dim3 b, size_t sm) {
  if (!trace_out) return;
  const char* name = kernel_name(f);
  fprintf(trace_out, "%s %u %u %zu\n", name, g.x, b.x, sm);
  fflush(trace_out);
}
hipError_t hipLaunchKernel(const void* f, dim3 g, dim3 b, void** args, size_t sm, hipStream_t s) {
  (void)s;
  ++n_launch;
  trace_launch(f, g, b, sm);
  if (n_pokes) poke_launch(kernel_name(f), args);
  if (__atomic_load_n(&fail_launches, __ATOMIC_SEQ_CST) > 0 && __atomic_fetch_sub(&fail_launches, 1, __ATOMIC_SEQ_CST) > 0) {
    sticky_error = hipErrorLaunchFailure;
    return hipErrorLaunchFailure;
  }
  return hipSuccess;
}
static void* fat_handle[4];
void** __hipRegisterFatBinary(const void* data) { (void)data; return fat_handle; }
void __hipRegisterFunction(void** m, const void* hf, char* df, const char* dn, unsigned tl, void* tid, void* bid, void* bd, void* gd, int* ws) {
  (void)m; (void)df; (void)tl; (void)tid; (void)bid; (void)bd; (void)gd; (void)ws;
  if (n_kernels < 1024) { kernels[n_kernels].host = hf; kernels[n_kernels].name = dn; ++n_kernels; }   // (before main: one thread)
}
void __hipRegisterVar(void** m, void* v, char* a, const char* b, int c, size_t d, int e, int f) { (void)m; (void)v; (void)a; (void)b; (void)c; (void)d; (void)e; (void)f; }
void __hipUnregisterFatBinary(void** m) { (void)m; }
static __thread dim3 cfg_g, cfg_b; static __thread size_t cfg_sm; static __thread hipStream_t cfg_s;
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t sm, hipStream_t s) { cfg_g = g; cfg_b = b; cfg_sm = sm; cfg_s = s; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* g, dim3* b, size_t* sm, hipStream_t* s) { *g = cfg_g; *b = cfg_b; *sm = cfg_sm; *s = cfg_s; return hipSuccess; }
long mockhip_launches(void) { return n_launch; }
