// The ownership rules of pomfret_amd/csrc/pf_call.h, on the host alone: HIP is
// tests/host/stub/hip/hip_runtime.h, which counts.  Built with
// -fsanitize=address,undefined by tests/test_pf_call_host.py: a double free, a
// leak or a use after free of a "device" array ends the program.
//   - alloc / release / destructor free each array exactly once;
//   - a released array is not freed;
//   - a failed alloc leaves nothing registered and no sticky error;
//   - the destructor waits for the stream before it frees, and destroys exactly
//     the events that were made;
//   - upload_hp replaces the view's tags only where it has copied them;
//   - the environment parsers refuse trailing text.
#include <stdio.h>
#include "../../pomfret_amd/csrc/pf_call.h"

static int failed = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); failed++; } } while (0)

static void reset() { stub() = stub_state(); }

int main() {
    // 1. every array freed once, after the stream is idle; events made on first use only
    reset();
    {
        pf_call call(nullptr);
        void *a = call.alloc(100), *b = call.alloc(0), *c = call.alloc(8);
        CHECK(a && b && c && stub().live.size() == 3);
        memset(b, 0xAB, 8);                          // "at least 8 bytes": the sanitizer checks the write
        CHECK(call.mark(0) && call.mark(2) && call.mark(0));
        CHECK(stub().events_made == 2);
        CHECK(call.ms(0, 2) == 1.5f);
        CHECK(stub().frees == 0);
    }
    CHECK(stub().frees == 3 && stub().bad_frees == 0 && stub().live.empty());
    CHECK(stub().syncs >= 1 && stub().syncs_at_first_free >= 1);
    CHECK(stub().events_destroyed == 2);

    // 2. a released array is the caller's
    reset();
    void *kept = nullptr;
    {
        pf_call call(nullptr);
        void *a = call.alloc(16);
        kept = call.alloc(32);
        void *c = call.alloc(64);
        CHECK(a && kept && c);
        call.release(kept);
        call.release(kept);                          // twice, and a stranger: no effect
        call.release(&failed);
        CHECK(call.owned.size() == 2);
    }
    CHECK(stub().frees == 2 && stub().bad_frees == 0 && stub().live.size() == 1 && stub().live.count(kept) == 1);
    memset(kept, 1, 32);                             // still alive
    CHECK(hipFree(kept) == hipSuccess && stub().live.empty());

    // 3. a failed alloc: NULL, nothing registered, no sticky error, the others still freed once
    reset();
    stub().fail_malloc_at = 1;
    {
        pf_call call(nullptr);
        void *a = call.alloc(24), *b = call.alloc(24), *c = call.alloc(24);
        CHECK(a && !b && c);
        CHECK(call.owned.size() == 2 && hipGetLastError() == hipSuccess);
    }
    CHECK(stub().frees == 2 && stub().bad_frees == 0 && stub().live.empty() && stub().events_destroyed == 0);

    // 4. the tags' override
    reset();
    {
        const uint8_t batch_tags[4] = {9, 9, 9, 9}, mine[4] = {0, 1, 254, 3};
        pf_calls_view v;
        memset(&v, 0, sizeof v);
        v.read_hp = batch_tags;
        pf_call call(nullptr);
        CHECK(call.upload_hp(nullptr, 4, v) == PF_OK && v.read_hp == batch_tags && stub().mallocs == 0);
        CHECK(call.upload_hp(mine, 0, v) == PF_OK && v.read_hp == batch_tags && stub().mallocs == 0);
        CHECK(call.upload_hp(mine, 4, v) == PF_OK && v.read_hp != batch_tags && v.read_hp != mine);
        CHECK(!memcmp(v.read_hp, mine, 4) && call.owned.size() == 1);
        const uint8_t *before = v.read_hp;
        stub().fail_copy = 1;
        CHECK(call.upload_hp(mine, 4, v) == PF_ERR_HIP && v.read_hp == before && call.owned.size() == 2);
        stub().fail_copy = 0;
        stub().fail_malloc_at = stub().mallocs;
        CHECK(call.upload_hp(mine, 4, v) == PF_ERR_NOMEM && v.read_hp == before && call.owned.size() == 2);
    }
    CHECK(stub().frees == 2 && stub().bad_frees == 0 && stub().live.empty());

    // 5. the environment parsers
    unsetenv("PF_T");
    CHECK(pf_env_pow2("PF_T", 64, 1024, 512) == 512 && pf_env_threads("PF_T", 256) == 256);
    const char *good[] = {"64", "128", "1024"}, *bad[] = {"64x", "", " 64", "+64", "-64", "96", "32", "2048", "x", "0x40", "64 "};
    for (const char *g : good) { setenv("PF_T", g, 1); CHECK(pf_env_pow2("PF_T", 64, 1024, 512) == (uint32_t)atoi(g)); }
    for (const char *b : bad) { setenv("PF_T", b, 1); CHECK(pf_env_pow2("PF_T", 64, 1024, 512) == 0); }
    for (const char *g : {"64", "256", "1024"}) { setenv("PF_T", g, 1); CHECK(pf_env_threads("PF_T", 256) == (uint32_t)atoi(g)); }
    for (const char *b : {"128", "0", "2048", "64x", ""}) { setenv("PF_T", b, 1); CHECK(pf_env_threads("PF_T", 256) == 0); }

    if (failed) return 1;
    printf("pf_call ok\n");
    return 0;
}
