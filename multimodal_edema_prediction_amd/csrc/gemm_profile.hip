// Live timing of the dominant kernel, the tag-1 (CXR-encoder) GEMM launches (bench.py roofline leg).
// mode 1: HIP events around every tag-1 launch, recorded on the stream the kernel is launched on (eager launches only:
//         events cannot be read back out of a replayed hipGraph on this ROCm);
// mode 2: an in-kernel launch clock — every tag-1 launch issued (or CAPTURED) while the mode is on gets a private slot of
//         four u64 in device memory; the first workgroup in and the last workgroup out stamp the 100-MHz wall clock, so a
//         slot always holds the begin / end of the LAST execution of its launch, replays of a captured graph included.
#include <algorithm>
#include <vector>

#include "common.h"
#include "gemm_profile.h"

namespace {
struct GemmProfile {
    int mode = 0;
    int collect_mode = 0;            // the last mode ARMED (1 or 2): what collect() reads — mode 0 only stops the gathering
    std::vector<hipEvent_t> ev;      // mode 1: pairs (start, stop)
    size_t used = 0;
    double flops = 0.0;
    unsigned long long* slots = nullptr;     // mode 2: device [MAX_SLOTS][4]
    std::vector<double> slot_flops;
    int slot_dev = -1;
};
constexpr size_t MAX_PROF_SLOTS = 4096;
GemmProfile g_prof;
}  // namespace

extern "C" int medp_gemm_profile_enable(int mode) {
    MEDP_CHECK_ARG(mode >= 0 && mode <= 2, "gemm_profile_enable: mode must be 0 (off), 1 (HIP events) or 2 (in-kernel clock)");
    if (mode == 1) {
        g_prof.used = 0;
        g_prof.flops = 0.0;
    }
    if (mode == 2) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (!g_prof.slots || g_prof.slot_dev != dev) {
            hipError_t e = hipMalloc((void**)&g_prof.slots, MAX_PROF_SLOTS * 4 * sizeof(unsigned long long));
            if (e != hipSuccess) { medp_set_error("gemm_profile_enable: %s", hipGetErrorString(e)); return (int)e; }
            g_prof.slot_dev = dev;
        }
        hipError_t e = hipMemset(g_prof.slots, 0, MAX_PROF_SLOTS * 4 * sizeof(unsigned long long));
        if (e != hipSuccess) { medp_set_error("gemm_profile_enable: %s", hipGetErrorString(e)); return (int)e; }
        g_prof.slot_flops.clear();
    }
    g_prof.mode = mode;      // mode 0 keeps what was gathered for collect()
    if (mode != 0) g_prof.collect_mode = mode;
    return 0;
}

extern "C" int medp_gemm_profile_collect(double* total_ms, long long* n_launches, double* total_flops) {
    MEDP_CHECK_ARG(total_ms && n_launches && total_flops, "gemm_profile_collect: null argument");
    double ms = 0.0;
    // Dispatch on the mode that was armed last, NOT on "slots exist": slots armed by an earlier mode-2 capture stay alive (their
    // graph may still be replayed) while a later mode-1 measurement of eager launches must report ITS events.
    if (g_prof.collect_mode == 2) {          // in-kernel clocks: the caller has synchronised the device
        const size_t n = g_prof.slot_flops.size();
        std::vector<unsigned long long> h(n * 4);
        hipError_t e = hipMemcpy(h.data(), g_prof.slots, n * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        if (e != hipSuccess) { medp_set_error("gemm_profile_collect: %s", hipGetErrorString(e)); return (int)e; }
        int khz = 100000;
        (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, g_prof.slot_dev);
        double fl = 0.0;
        long long cnt = 0;
        for (size_t i = 0; i < n; ++i) {
            if (h[4 * i + 1] <= h[4 * i]) continue;      // never executed
            ms += (double)(h[4 * i + 1] - h[4 * i]) / (double)khz;
            fl += g_prof.slot_flops[i];
            ++cnt;
        }
        *total_ms = ms;
        *n_launches = cnt;
        *total_flops = fl;
        return 0;
    }
    for (size_t i = 0; i + 1 < g_prof.used; i += 2) {
        hipError_t e = hipEventSynchronize(g_prof.ev[i + 1]);
        if (e != hipSuccess) { medp_set_error("gemm_profile_collect: %s", hipGetErrorString(e)); return (int)e; }
        float t = 0.f;
        e = hipEventElapsedTime(&t, g_prof.ev[i], g_prof.ev[i + 1]);
        if (e != hipSuccess) { medp_set_error("gemm_profile_collect: %s", hipGetErrorString(e)); return (int)e; }
        ms += t;
    }
    *total_ms = ms;
    *n_launches = (long long)(g_prof.used / 2);
    *total_flops = g_prof.flops;
    g_prof.used = 0;
    g_prof.flops = 0.0;
    return 0;
}

// Debug hook (NOT part of the C ABI in include/medp_hip.h; tools/time_branches.py): the raw mode-2 stamps, slot i ->
// out[2 i] = first workgroup in, out[2 i + 1] = last workgroup out (ticks of the wall clock, *khz per ms), in launch order.
extern "C" int medp_dbg_gemm_profile_raw(unsigned long long* out, int max_slots, int* n_slots, int* khz) {
    const int n = (int)std::min(g_prof.slot_flops.size(), (size_t)std::max(max_slots, 0));
    std::vector<unsigned long long> h((size_t)n * 4);
    if (n > 0 && hipMemcpy(h.data(), g_prof.slots, (size_t)n * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    for (int i = 0; i < n; ++i) { out[2 * i] = h[4 * i]; out[2 * i + 1] = h[4 * i + 1]; }
    *n_slots = n;
    *khz = 100000;
    (void)hipDeviceGetAttribute(khz, hipDeviceAttributeWallClockRate, g_prof.slot_dev);
    return 0;
}

// The dispatcher's side: a begin / end pair around every tag-1 launch.  `tile256`: the launch takes the 256-tile kernels, the only
// ones that stamp a mode-2 slot (returned, or nullptr: mode 2 off, no slot left, another kernel family).
int medp_gemm_profile_begin(bool tile256, double flops, void* stream, unsigned long long** slot) {
    *slot = nullptr;
    if (g_prof.mode == 2 && tile256 && g_prof.slot_flops.size() < MAX_PROF_SLOTS) {
        *slot = g_prof.slots + 4 * g_prof.slot_flops.size();
        g_prof.slot_flops.push_back(flops);
    }
    if (g_prof.mode == 1) {
        if (g_prof.used + 2 > g_prof.ev.size()) {
            for (int i = 0; i < 2; ++i) {
                hipEvent_t e;
                if (hipEventCreate(&e) != hipSuccess) { medp_set_error("gemm profile: hipEventCreate failed"); return 1; }
                g_prof.ev.push_back(e);
            }
        }
        hipEventRecord(g_prof.ev[g_prof.used], (hipStream_t)stream);
    }
    return 0;
}

void medp_gemm_profile_end(double flops, void* stream) {
    if (g_prof.mode != 1) return;
    hipEventRecord(g_prof.ev[g_prof.used + 1], (hipStream_t)stream);
    g_prof.used += 2;
    g_prof.flops += flops;
}
