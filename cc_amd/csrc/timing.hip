// Per-kernel timing registry (tools build only; include/ccengine.h) and cc_is_tools_build.  Off unless cc_timing_enable(1) was
// called on this process (autograd runs the backward pass on its own threads, so the registry is process-wide behind a mutex).
// cctiming::Scope (conv_internal.h) is what the convolution units put around the MAIN device kernel of a call: HIP events on its
// own stream, so the reported duration is the kernel's (what rocprofv3 --kernel-trace shows), not the C-ABI call's.
#include <stdio.h>
#include "cc_common.h"
#include "conv_internal.h"
#include "../../include/ccengine.h"
#include <vector>
#include <string>
#include <mutex>

#ifdef CC_TOOLS
namespace cctiming {
struct Rec { std::string name; double gflop; hipEvent_t e0, e1; };
static std::vector<Rec>* recs = nullptr;
static std::mutex mtx;
Scope::Scope(const char* name, double gflop, hipStream_t st, bool active) : s(st) {
    if (!recs || !active) return;
    hipEvent_t e0 = nullptr;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    {
        std::lock_guard<std::mutex> lk(mtx);
        if (!recs) return;
        recs->push_back(Rec{name, gflop, e0, e1});
    }
    (void)hipEventRecord(e0, s);
}
Scope::~Scope() { if (e1) (void)hipEventRecord(e1, s); }
}  // namespace cctiming
#endif

extern "C" {

#ifdef CC_TOOLS
int cc_timing_enable(int on) {
    std::lock_guard<std::mutex> lk(cctiming::mtx);
    if (on && !cctiming::recs) cctiming::recs = new std::vector<cctiming::Rec>();
    if (on) cctiming::recs->reserve(4096);
    if (!on && cctiming::recs) {
        for (auto& r : *cctiming::recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
        delete cctiming::recs;
        cctiming::recs = nullptr;
    }
    return CC_OK;
}

int cc_timing_collect(void* out_host, int cap) {
    char* out = (char*)out_host;
    int len = 0;
    if (!cctiming::recs || cap <= 0) return 0;
    struct Agg { std::string name; int n; double ms, gf; };
    std::vector<Agg> agg;
    for (auto& r : *cctiming::recs) {
        float ms = 0.f;
        (void)hipEventSynchronize(r.e1);
        (void)hipEventElapsedTime(&ms, r.e0, r.e1);
        Agg* a = nullptr;
        for (auto& x : agg) if (x.name == r.name) { a = &x; break; }
        if (!a) { agg.push_back(Agg{r.name, 0, 0.0, 0.0}); a = &agg.back(); }
        a->n++; a->ms += ms; a->gf += r.gflop;
    }
    for (auto& a : agg) {
        const int k = snprintf(out + len, cap - len, "%s\t%d\t%.6f\t%.6f\n", a.name.c_str(), a.n, a.ms, a.gf);
        if (k < 0 || k >= cap - len) break;
        len += k;
    }
    cc_timing_enable(0);       // (takes the lock itself)
    return len;
}
#else
/* product build: no timing registry (the library keeps no state); the tools build records */
int cc_timing_enable(int on) { return on ? CC_ERR_ARG : CC_OK; }
int cc_timing_collect(void* out_host, int cap) { (void)out_host; (void)cap; return 0; }
#endif

/* 1 for the tools build (switches + timing compiled in), 0 for the product library */
int cc_is_tools_build(void) {
#ifdef CC_TOOLS
    return 1;
#else
    return 0;
#endif
}

}  // extern "C"
