// A host-only stand-in for the HIP entry points pomfret_amd/csrc/pf_call.h
// uses, for tests/host/pf_call_check.cpp: device arrays are malloc'ed blocks,
// every call is counted, and failures are injected through the counters below.
#ifndef PF_STUB_HIP_RUNTIME_H
#define PF_STUB_HIP_RUNTIME_H
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <set>

typedef int hipError_t;
#define hipSuccess 0
#define hipErrorOutOfMemory 2
typedef struct stub_stream *hipStream_t;
typedef struct stub_event *hipEvent_t;
struct stub_event { int recorded; };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };

struct stub_state {
    std::set<void *> live;         // device arrays not yet freed
    int mallocs = 0, frees = 0, bad_frees = 0, syncs = 0, events_made = 0, events_destroyed = 0, copies = 0;
    int fail_malloc_at = -1;       // the malloc (counted from 0) that fails
    int fail_copy = 0;
    hipError_t sticky = hipSuccess;
    int syncs_at_first_free = -1;  // the destructor waits for the stream before it frees
};
inline stub_state &stub() { static stub_state s; return s; }

inline hipError_t hipMalloc(void **p, size_t bytes) {
    stub_state &s = stub();
    if (s.mallocs++ == s.fail_malloc_at || bytes < 8) { *p = nullptr; return s.sticky = hipErrorOutOfMemory; }
    *p = malloc(bytes);
    s.live.insert(*p);
    return hipSuccess;
}
inline hipError_t hipFree(void *p) {
    stub_state &s = stub();
    if (s.syncs_at_first_free < 0) s.syncs_at_first_free = s.syncs;
    s.frees++;
    if (!s.live.erase(p)) { s.bad_frees++; return 1; }     // a double free or a pointer that was never ours
    free(p);
    return hipSuccess;
}
inline hipError_t hipGetLastError() { const hipError_t e = stub().sticky; stub().sticky = hipSuccess; return e; }
inline hipError_t hipStreamSynchronize(hipStream_t) { stub().syncs++; return hipSuccess; }
inline hipError_t hipEventCreate(hipEvent_t *e) { *e = new stub_event{0}; stub().events_made++; return hipSuccess; }
inline hipError_t hipEventDestroy(hipEvent_t e) { delete e; stub().events_destroyed++; return hipSuccess; }
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { e->recorded++; return hipSuccess; }
inline hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b) {
    *ms = a->recorded && b->recorded ? 1.5f : 0.0f;
    return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind, hipStream_t) {
    stub().copies++;
    if (stub().fail_copy) return 1;
    memcpy(dst, src, n);
    return hipSuccess;
}
#endif
