// fs_objects.h - the registry of a context's live device objects (history rings, averages, tracer sets, ...: everything behind an opaque handle
// except the fields) and the one check of a handle against it.  No HIP in here: what an entry owns is a deleter, so the host compiler builds this
// header on its own for the CPU tests (fs_objects_host.cpp).
#pragma once
#include <functional>
#include <map>
#include <memory>
#include <vector>

namespace fs {

struct Objects {
    struct Entry { int kind; void *obj; void (*destroy)(void *); };
    std::map<const void *, Entry> live;      // by the handle's pointer value, exactly as the caller holds it
    // a *_free during a hipGraph capture (neither a synchronisation nor hipFree is legal there: either invalidates the capture) leaves its
    // release here; fs_graph_end and fs_destroy run the list in the order of the calls
    std::vector<std::function<void()>> deferred;

    // the registry takes the object over; the handle the caller gets
    template <typename T> T *adopt(std::unique_ptr<T> obj, int kind)
    {
        live[obj.get()] = Entry{kind, obj.get(), [](void *p) { delete static_cast<T *>(p); }};
        return obj.release();
    }
    // THE handle check: the pointer value is looked up, then the entry's kind compared - `h` itself is never read, so a stale handle (freed, of
    // another context, of another kind) is refused without touching freed memory
    bool holds(const void *h, int kind) const
    {
        const auto it = live.find(h);
        return it != live.end() && it->second.kind == kind;
    }
    // takes a live object out and releases it: at once, after quiesce(), or - `defer` - when run_deferred() next runs.  false: no live handle of this kind
    template <typename Q> bool free(const void *h, int kind, bool defer, Q quiesce)
    {
        if (!holds(h, kind)) return false;
        const Entry e = live[h];
        live.erase(h);
        if (defer) deferred.push_back([e] { e.destroy(e.obj); });
        else { quiesce(); e.destroy(e.obj); }
        return true;
    }
    void run_deferred()
    {
        for (auto &release : deferred) release();
        deferred.clear();
    }
    // the end of the context: whatever is still live (an object whose free was deferred is not: it is released by run_deferred alone)
    void release_live()
    {
        for (auto &kv : live) kv.second.destroy(kv.second.obj);
        live.clear();
    }
};

}  // namespace fs
