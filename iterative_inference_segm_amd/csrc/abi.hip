// Status strings / version of the C ABI (include/iiseg.h); launch profiling state; the argument checks of the
// C8 adjoint entries.
#include <stdint.h>
#include <mutex>
#include <vector>
#include "common.h"
#include "c8_common.h"

namespace {
std::mutex g_prof_mu;
std::vector<hipEvent_t> g_prof_ev;      // pairs (start, stop), created once and reused
int g_prof_on = 0, g_prof_n = 0, g_prof_cap = 0;
}  // namespace

extern "C" int iiseg_prof_next(hipEvent_t* start, hipEvent_t* stop) {
    if (!g_prof_on) return 0;
    std::lock_guard<std::mutex> g(g_prof_mu);
    if (!g_prof_on || g_prof_n >= g_prof_cap) return 0;
    *start = g_prof_ev[2 * g_prof_n];
    *stop = g_prof_ev[2 * g_prof_n + 1];
    ++g_prof_n;
    return 1;
}

extern "C" int iiseg_profile_begin(int capacity) {
    if (capacity <= 0) return IISEG_ERR_SHAPE;
    std::lock_guard<std::mutex> g(g_prof_mu);
    while ((int)g_prof_ev.size() < 2 * capacity) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return IISEG_ERR_LAUNCH;
        g_prof_ev.push_back(e);
    }
    g_prof_cap = capacity;
    g_prof_n = 0;
    g_prof_on = 1;
    return IISEG_OK;
}

extern "C" int iiseg_profile_count(void) { return g_prof_on ? g_prof_n : -1; }

extern "C" int iiseg_profile_end(float* ms, int capacity) {
    std::lock_guard<std::mutex> g(g_prof_mu);
    if (!g_prof_on) return -1;
    g_prof_on = 0;
    const int n = g_prof_n < capacity ? g_prof_n : capacity;
    for (int i = 0; i < n; ++i) {
        if (hipEventSynchronize(g_prof_ev[2 * i + 1]) != hipSuccess ||
            hipEventElapsedTime(&ms[i], g_prof_ev[2 * i], g_prof_ev[2 * i + 1]) != hipSuccess)
            return IISEG_ERR_LAUNCH;
    }
    return n;
}

extern "C" const char* iiseg_strerror(int status) {
    switch (status) {
        case IISEG_OK: return "ok";
        case IISEG_ERR_NULL: return "required pointer is NULL";
        case IISEG_ERR_SHAPE: return "inconsistent or unsupported shape";
        case IISEG_ERR_ALIGN: return "pointer is not 16-byte aligned";
        case IISEG_ERR_LAUNCH: return "kernel launch failed";
        case IISEG_ERR_UNSUPPORTED: return "no kernel variant implements this request";
        default: return "unknown iiseg status";
    }
}

extern "C" const char* iiseg_last_hip_error(void) {
    return hipGetErrorString((hipError_t)iiseg_hip_error_slot());
}

// ---- the element-wise adjoints of the standard DAE's C8 backward walk (kernels: c8_grad.hip) ----
namespace {
// a pooled-coordinate window of C8 planes: B images of C8n chunks (whole 16-channel groups: C8n even)
int c8_window_status(int B, int C8n, int h2, int w2, int y0, int x0, int wh, int ww) {
    if (B <= 0 || C8n <= 0 || (C8n & 1) || h2 <= 0 || w2 <= 0 || wh <= 0 || ww <= 0 || y0 < 0 || x0 < 0 ||
        y0 > h2 - wh || x0 > w2 - ww)
        return IISEG_ERR_SHAPE;
    return IISEG_OK;
}
}  // namespace

extern "C" int iiseg_depool_bwd_c8(void* stream, const void* gu, const uint8_t* mask, const void* gate, void* out,
                                   int B, int C8n, int PH, int PW, int h2, int w2, int y0, int x0, int wh, int ww) {
    if (!gu || !mask || !out) return IISEG_ERR_NULL;
    const int st = c8_window_status(B, C8n, h2, w2, y0, x0, wh, ww);
    if (st) return st;
    if (PH < 2 * (int64_t)h2 || PW < 2 * (int64_t)w2) return IISEG_ERR_SHAPE;
    if (((uintptr_t)gu & 15) || ((uintptr_t)gate & 15) || ((uintptr_t)out & 15) || ((uintptr_t)mask & 7))
        return IISEG_ERR_ALIGN;
    if (out == gu || out == gate) return IISEG_ERR_UNSUPPORTED;      // not in place: four reads per element
    return iiseg::depool_bwd_c8_launch(stream, gu, mask, gate, out, (int64_t)B * C8n, PH, PW, h2, w2, y0, x0, wh,
                                       ww);
}

extern "C" int iiseg_relu_gate_c8(void* stream, const void* g, const void* pooled, void* out, int B, int C8n,
                                  int h2, int w2, int y0, int x0, int wh, int ww) {
    if (!g || !pooled || !out) return IISEG_ERR_NULL;
    const int st = c8_window_status(B, C8n, h2, w2, y0, x0, wh, ww);
    if (st) return st;
    if (((uintptr_t)g & 15) || ((uintptr_t)pooled & 15) || ((uintptr_t)out & 15)) return IISEG_ERR_ALIGN;
    if (out == pooled) return IISEG_ERR_UNSUPPORTED;                 // (out == g is fine: element-wise)
    return iiseg::relu_gate_c8_launch(stream, g, pooled, out, (int64_t)B * C8n, h2, w2, y0, x0, wh, ww);
}

extern "C" int iiseg_abi_version(void) { return 34; }
extern "C" const char* iiseg_target_arch(void) { return "gfx950"; }
