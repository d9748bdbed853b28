// pf_call.h -- the scope of one device call of the pileup family (host only):
// the context's stream, the call's temporary device arrays and its timing
// events.  A function declares one pf_call after the host objects that the
// stream may still write to (the result, staging vectors), so that on every
// return the destructor first waits for the stream, then frees what the call
// still owns and destroys the events, and only then those objects go.  What
// becomes of the result on failure stays with the function: the scope knows no
// result types.  Also the parsers of the test-only environment knobs.
#ifndef PF_CALL_H
#define PF_CALL_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pf_device.h"
#include "../../include/pomfret_amd.h"

#define PF_CALL_EVENTS 4

struct pf_call {
    hipStream_t st;
    std::vector<void *> owned;                 // this call's device arrays
    hipEvent_t ev[PF_CALL_EVENTS] = {nullptr, nullptr, nullptr, nullptr};

    explicit pf_call(hipStream_t stream) : st(stream) {}
    pf_call(const pf_call &) = delete;
    pf_call &operator=(const pf_call &) = delete;
    ~pf_call() {
        (void)hipStreamSynchronize(st);
        for (void *p : owned) (void)hipFree(p);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }

    // a device array of at least 8 bytes that lives as long as the call; NULL
    // (nothing registered, no sticky error left) where there is no memory
    void *alloc(size_t bytes) {
        void *p = nullptr;
        try { owned.reserve(owned.size() + 1); } catch (...) { return nullptr; }
        if (hipMalloc(&p, bytes < 8 ? 8 : bytes) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        owned.push_back(p);
        return p;
    }

    // p outlives the call: the caller frees it
    void release(void *p) {
        for (size_t i = 0; i < owned.size(); i++)
            if (owned[i] == p) { owned.erase(owned.begin() + (long)i); return; }
    }

    // record event i on the stream (created on first use); false: a HIP error
    bool mark(int i) {
        if (!ev[i] && hipEventCreate(&ev[i]) != hipSuccess) { ev[i] = nullptr; return false; }
        return hipEventRecord(ev[i], st) == hipSuccess;
    }
    // the milliseconds between two marks that the stream has passed
    float ms(int i, int j) {
        float t = 0.0f;
        (void)hipEventElapsedTime(&t, ev[i], ev[j]);
        (void)hipGetLastError();
        return t;
    }

    // the caller's tags in place of the batch's: read_hp NULL (or R == 0) keeps the view as it is
    int upload_hp(const uint8_t *read_hp, uint32_t R, pf_calls_view &v) {
        if (!read_hp || !R) return PF_OK;
        void *p = alloc(R);
        if (!p) return PF_ERR_NOMEM;
        if (hipMemcpyAsync(p, read_hp, R, hipMemcpyHostToDevice, st) != hipSuccess) return PF_ERR_HIP;
        v.read_hp = static_cast<const uint8_t *>(p);
        return PF_OK;
    }
};

// NAME=<n> (tests: tile and block edges at tiny shapes), n a power of two in
// [lo, hi] written in digits alone; dflt where the variable is not set, 0 for
// any other value
static inline uint32_t pf_env_pow2(const char *name, long lo, long hi, uint32_t dflt) {
    const char *e = getenv(name);
    if (!e) return dflt;
    if (*e < '0' || *e > '9') return 0;
    char *end = nullptr;
    const long n = strtol(e, &end, 10);
    if (*end || n < lo || n > hi || (n & (n - 1))) return 0;
    return (uint32_t)n;
}

// NAME=<64|256|1024>, a workgroup size (tests); dflt where the variable is not set, 0 for any other value
static inline uint32_t pf_env_threads(const char *name, uint32_t dflt) {
    const char *e = getenv(name);
    if (!e) return dflt;
    if (!strcmp(e, "64")) return 64;
    if (!strcmp(e, "256")) return 256;
    if (!strcmp(e, "1024")) return 1024;
    return 0;
}

#endif
