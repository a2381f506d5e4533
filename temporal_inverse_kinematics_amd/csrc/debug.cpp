// debug.cpp — the debug hooks of libtik.so: guard zones (TIK_GUARD),
// per-launch checksums (TIK_CHECKSUM), the profiler scope, and the phase
// traces of the bf16x3 kernels (TIK_X_TRACE).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <mutex>

#include "misc.h"
#include "model.h"

namespace tik_host {
std::atomic<int> g_alloc_fill{-1};
thread_local Profiler* g_prof = nullptr;

bool guard_mode() {
    static const bool on = getenv("TIK_GUARD") && getenv("TIK_GUARD")[0] == '1';
    return on;
}
static std::mutex g_guard_mu;
static std::map<void*, size_t> g_guard_bufs;   // base -> payload bytes
void guard_register(void* base, size_t bytes) {
    std::lock_guard<std::mutex> l(g_guard_mu);
    g_guard_bufs[base] = bytes;
}
void guard_unregister(void* base) {
    std::lock_guard<std::mutex> l(g_guard_mu);
    g_guard_bufs.erase(base);
}

// TIK_CHECKSUM=1: after every annotated launch, synchronise and record a
// checksum of its output buffer
static bool checksum_mode() {
    static const bool on = getenv("TIK_CHECKSUM") != nullptr;
    return on;
}
static std::string g_cks;
static unsigned long long* g_cks_dev = nullptr;

ProfScope::~ProfScope() {
    if (g_prof) g_prof->end(i, st);
    if (checksum_mode() && op) {
        if (!g_cks_dev) (void)hipMalloc(&g_cks_dev, 8);
        unsigned long long h = 0;
        (void)hipMemsetAsync(g_cks_dev, 0, 8, st);
        (void)tik::launch_checksum(op, obytes, g_cks_dev, st);
        (void)hipMemcpyAsync(&h, g_cks_dev, 8, hipMemcpyDeviceToHost, st);
        (void)hipStreamSynchronize(st);
        char b[160];
        snprintf(b, sizeof(b), "%s:%llx;", lab, h);
        g_cks += b;
    }
}

// launch(trace): with TIK_X_TRACE set, trace points at `slots` zeroed 64-bit
// stamps, which go to report() once the stream has synchronised; else null
template <class Launch, class Report>
static hipError_t launch_traced(size_t slots, hipStream_t st, Launch launch, Report report) {
    static const bool on = getenv("TIK_X_TRACE") != nullptr;
    if (!on) return launch(nullptr);
    unsigned long long* d = nullptr;
    hipError_t e = hipMalloc(&d, slots * 8);
    if (e != hipSuccess) return e;
    (void)hipMemset(d, 0, slots * 8);
    e = launch(d);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    std::vector<unsigned long long> h(slots);
    if (e == hipSuccess) e = hipMemcpy(h.data(), d, slots * 8, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    report(h);
    return e;
}

// xgemm.hip: 8 slots per workgroup (s_memtime cycles)
hipError_t launch_xgemm_traced(tik::XArgs a, int bn, int epi, hipStream_t st, const char* label) {
    const int rt = tik::xgemm_tile_rows(epi);
    const long long nwg = (long long)((a.M + rt - 1) / rt) * ((a.Nc + bn - 1) / bn);
    return launch_traced(nwg * 8, st,
        [&](unsigned long long* d) { a.trace = d; return tik::launch_xgemm(a, bn, epi, st); },
        [&](const std::vector<unsigned long long>& h) {
            double s[5] = {0, 0, 0, 0, 0}, n = 0, ks = 0;
            for (long long w = 0; w < nwg; ++w) {
                if (!h[8 * w + 6]) continue;
                n += 1; ks = (double)h[8 * w + 5];
                for (int k = 0; k < 5; ++k) s[k] += (double)h[8 * w + k];
            }
            n = std::max(1.0, n);
            fprintf(stderr, "XTRACE %-10s wg %6.0f ksteps %3.0f | cycles/wg: prologue %7.0f main %8.0f epi %7.0f | "
                    "barrier %7.0f vmwait %7.0f | main/kstep %6.0f\n", label, n, ks, s[0] / n, s[1] / n, s[2] / n,
                    s[3] / n, s[4] / n, s[1] / n / std::max(1.0, ks));
        });
}

// xgraph.hip: 16 stamps per workgroup (waves 0 and 4)
hipError_t launch_xgraph_traced(tik::XGraphArgs a, int ncu, hipStream_t st, const char* label) {
    return launch_traced((size_t)ncu * 16, st,
        [&](unsigned long long* d) { a.trace = d; return tik::launch_xgraph(a, ncu, st); },
        [&](const std::vector<unsigned long long>& h) {
            double s0[8] = {0}, s4[8] = {0}, n = 0;
            for (int w = 0; w < ncu; ++w) {
                if (!h[16 * w + 6]) continue;
                n += 1;
                for (int k = 0; k < 8; ++k) { s0[k] += (double)h[16 * w + k]; s4[k] += (double)h[16 * w + 8 + k]; }
            }
            const double ns = std::max(1.0, s0[6]);
            fprintf(stderr, "XGTRACE %-8s wgs %4.0f steps/wg %5.1f total/wg %8.0f | per step, wave0: bar %6.0f mfma0-3 %6.0f split %6.0f load %6.0f mfma4-16 %6.0f epi %6.0f"
                    " | wave4: bar %6.0f mfma0-3 %6.0f split %6.0f load %6.0f mfma4-16 %6.0f epi %6.0f\n", label, n, s0[6] / std::max(1.0, n),
                    s0[7] / std::max(1.0, n), s0[0] / ns, s0[1] / ns, s0[2] / ns, s0[3] / ns, s0[4] / ns, s0[5] / ns, s4[0] / ns, s4[1] / ns,
                    s4[2] / ns, s4[3] / ns, s4[4] / ns, s4[5] / ns);
        });
}

// xblock.hip (a -DTIK_XTRACE build): 24 stamps per workgroup, per-phase sums
hipError_t launch_xblock_traced(tik::XBlkArgs a, bool raw, int ncu, hipStream_t st, const char* label) {
    return launch_traced((size_t)ncu * 24, st,
        [&](unsigned long long* d) { a.trace = d; return tik::launch_xblock(a, raw, ncu, st); },
        [&](const std::vector<unsigned long long>& h) {
            double s0[8] = {0}, s4[8] = {0}, nt = 0;
            for (int w = 0; w < ncu; ++w) {
                if (!h[24 * w + 9]) continue;
                nt += (double)h[24 * w + 8];
                for (int k = 0; k < 8; ++k) { s0[k] += (double)h[24 * w + k]; s4[k] += (double)h[24 * w + 12 + k]; }
            }
            nt = std::max(1.0, nt);
            fprintf(stderr, "XBTRACE %-8s tiles %6.0f | per tile, wave0: start %6.0f G+mix %6.0f zbar %6.0f res %6.0f bar+dma %6.0f T %6.0f endbar %6.0f"
                    " | wave4: start %6.0f G+mix %6.0f zbar %6.0f res %6.0f bar+dma %6.0f T %6.0f endbar %6.0f\n", label, nt,
                    s0[0] / nt, s0[1] / nt, s0[2] / nt, (s0[3] + s0[6]) / nt, s0[7] / nt, s0[4] / nt, s0[5] / nt, s4[0] / nt, s4[1] / nt,
                    s4[2] / nt, (s4[3] + s4[6]) / nt, s4[7] / nt, s4[4] / nt, s4[5] / nt);
        });
}

}  // namespace tik_host
using namespace tik_host;

extern "C" {

int tik_debug_checksums(char* buf, int len) {
    if (!checksum_mode()) return fail(TIK_E_INVALID, "TIK_CHECKSUM is not set");
    const int n = (int)g_cks.size();
    if (buf && len > 0) {
        strncpy(buf, g_cks.c_str(), len - 1);
        buf[len - 1] = 0;
    }
    g_cks.clear();
    return n;
}

int tik_debug_check_guards(void) {
    if (!guard_mode()) return fail(TIK_E_INVALID, "TIK_GUARD=1 is not set");
    HIP_TRY(hipDeviceSynchronize());
    std::lock_guard<std::mutex> l(g_guard_mu);
    std::vector<unsigned char> h(GUARD_BYTES);
    int bad = 0;
    std::string rep;
    for (const auto& kv : g_guard_bufs) {
        const char* base = static_cast<const char*>(kv.first);
        for (int side = 0; side < 2; ++side) {
            const char* gp = side == 0 ? base : base + GUARD_BYTES + kv.second;
            HIP_TRY(hipMemcpy(h.data(), gp, GUARD_BYTES, hipMemcpyDeviceToHost));
            size_t first = GUARD_BYTES, last = 0, cnt = 0;
            bool clean = true;   // the common case, a word at a time (a handle has hundreds of guards)
            for (size_t i = 0; i < GUARD_BYTES && clean; i += 8) {
                unsigned long long w;
                memcpy(&w, h.data() + i, 8);
                clean = w == 0xA5A5A5A5A5A5A5A5ull;
            }
            for (size_t i = 0; i < GUARD_BYTES && !clean; ++i)
                if (h[i] != 0xA5) { first = std::min(first, i); last = i; ++cnt; }
            if (cnt) {
                ++bad;
                char b[256];
                snprintf(b, sizeof(b), "[buf %p payload %zu B: %s guard, %zu bytes changed at +%zu..+%zu] ", (const void*)(base + GUARD_BYTES),
                         kv.second, side == 0 ? "front" : "back", cnt, first, last);
                rep += b;
                HIP_TRY(hipMemset(const_cast<char*>(gp), 0xA5, GUARD_BYTES));
            }
        }
    }
    g_err = rep;
    return bad;
}

int tik_debug_alloc_fill(void) { return g_alloc_fill.load(); }

}  // extern "C"
