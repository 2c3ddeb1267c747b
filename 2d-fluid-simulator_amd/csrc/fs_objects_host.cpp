// fs_objects_host.cpp - libfs_objects_host.so: the object registry and handle check of fs_objects.h behind C functions, for
// tests/test_objects_cpu.py.  Host compiler only, no HIP; test infrastructure - the product never loads it.  The objects registered here record
// their destruction in a log, in order.  -DFS_OBJECTS_HOST_MAIN adds a main() that walks the same cases, for a run under the host sanitizers.
#include "fs_objects.h"

namespace {
std::vector<int> g_log;      // ids, in the order their objects were destroyed
struct Probe {
    int id;
    ~Probe() { g_log.push_back(id); }
};
}  // namespace

extern "C" {

void *fs_objects_host_new(void) { return new fs::Objects(); }

// as fs_destroy: whatever is live, then what a capture that never ended left behind
void fs_objects_host_destroy(void *reg)
{
    fs::Objects *o = static_cast<fs::Objects *>(reg);
    o->release_live();
    o->run_deferred();
    delete o;
}

void *fs_objects_host_create(void *reg, int kind, int id)
{
    auto p = std::make_unique<Probe>();
    p->id = id;
    return static_cast<fs::Objects *>(reg)->adopt(std::move(p), kind);
}

int fs_objects_host_holds(const void *reg, const void *h, int kind) { return static_cast<const fs::Objects *>(reg)->holds(h, kind) ? 1 : 0; }

// as object_free (fs_host.h): 0 for a null handle and for a live one of this kind, -1 for every other
int fs_objects_host_free(void *reg, void *h, int kind, int capturing)
{
    if (!h) return 0;
    return static_cast<fs::Objects *>(reg)->free(h, kind, capturing != 0, [] {}) ? 0 : -1;
}

void fs_objects_host_run_deferred(void *reg) { static_cast<fs::Objects *>(reg)->run_deferred(); }

// the destruction log: its length; up to `cap` ids into `out`
int fs_objects_host_log(int *out, int cap)
{
    for (int k = 0; k < cap && k < (int)g_log.size(); ++k) out[k] = g_log[k];
    return (int)g_log.size();
}
void fs_objects_host_log_clear(void) { g_log.clear(); }

}  // extern "C"

#ifdef FS_OBJECTS_HOST_MAIN
#include <cstdio>
#include <cstdlib>
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)
int main()
{
    void *a = fs_objects_host_new(), *b = fs_objects_host_new();
    void *h0 = fs_objects_host_create(a, 0, 10), *h1 = fs_objects_host_create(a, 1, 11), *h2 = fs_objects_host_create(a, 0, 12);
    void *h3 = fs_objects_host_create(a, 1, 13), *hb = fs_objects_host_create(b, 0, 20);
    CHECK(fs_objects_host_holds(a, h0, 0) && !fs_objects_host_holds(a, h0, 1) && !fs_objects_host_holds(b, h0, 0) && !fs_objects_host_holds(a, hb, 0));
    CHECK(fs_objects_host_free(b, h0, 0, 0) == -1 && fs_objects_host_free(a, h0, 1, 0) == -1 && fs_objects_host_holds(a, h0, 0));
    CHECK(fs_objects_host_free(a, nullptr, 0, 0) == 0);
    CHECK(fs_objects_host_free(a, h0, 0, 0) == 0 && g_log == std::vector<int>({10}));
    // h0 is freed memory from here on: every lookup below must get by without reading it
    CHECK(!fs_objects_host_holds(a, h0, 0) && !fs_objects_host_holds(a, h0, 1) && fs_objects_host_free(a, h0, 0, 0) == -1 && fs_objects_host_free(a, h0, 0, 1) == -1);
    // "inside a capture": nothing is destroyed before the deferred list runs, then in the order of the calls
    CHECK(fs_objects_host_free(a, h3, 1, 1) == 0 && fs_objects_host_free(a, h1, 1, 1) == 0 && g_log.size() == 1);
    CHECK(!fs_objects_host_holds(a, h3, 1) && fs_objects_host_free(a, h3, 1, 1) == -1);
    fs_objects_host_run_deferred(a);
    CHECK(g_log == std::vector<int>({10, 13, 11}));
    CHECK(!fs_objects_host_holds(a, h1, 1) && fs_objects_host_free(a, h1, 1, 0) == -1);
    // the end of a registry: the live object once, what was deferred and run not again; a deferred free that never ran, once
    CHECK(fs_objects_host_free(b, hb, 0, 1) == 0);
    fs_objects_host_destroy(a);
    CHECK(g_log == std::vector<int>({10, 13, 11, 12}));
    (void)h2;
    fs_objects_host_destroy(b);
    CHECK(g_log == std::vector<int>({10, 13, 11, 12, 20}));
    std::puts("fs_objects_host: ok");
    return 0;
}
#endif
