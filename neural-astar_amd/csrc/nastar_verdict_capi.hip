// nastar_verdict_capi.hip -- the C ABI of include/nastar_verdict.h: the proof that a batch is solvable, launched beside its search.  A
// translation unit of its own: nothing here touches the search, replay or encoder kernels.
#include <hip/hip_runtime.h>

#include <mutex>

#include "nastar_verdict.hip.h"
#include "nastar_host.hip.h"
#include "../../include/nastar_verdict.h"

using namespace nastar;

namespace {

// the side stream of one device, the event that orders it behind the caller's stream, and the grid (one wavefront per SIMD); made at the
// first launch on that device, kept for the life of the library
struct ProofLane {
    hipStream_t stream = nullptr;
    hipEvent_t event = nullptr;
    int max_grid = 0;
};
constexpr int kMaxDevices = 64;
ProofLane g_lanes[kMaxDevices];
std::mutex g_lanes_mutex;

int proof_lane(ProofLane** out)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
    if (dev < 0 || dev >= kMaxDevices) return NASTAR_ERR_UNSUPPORTED;
    ProofLane& l = g_lanes[dev];
    if (l.stream == nullptr) {
        int cus = 0;
        if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return hip_fail(e, "hipDeviceGetAttribute");
        // The event only orders the side stream behind the caller's stream ON THIS DEVICE: nobody synchronises with it from the host or asks
        // it for a time.  Recorded with the default flags, its marker packet sits between two consecutive search launches of the caller's
        // stream and performs a system-scope release there (L2 written back and invalidated for the host) -- 2.4 us per checked step,
        // for a consumer that is a kernel of the same device.  hipEventDisableSystemFence leaves the marker as the plain barrier it needs to
        // be: what earlier kernels of the stream wrote is released at device scope by those kernels' own ends, and the proof kernel begins
        // with its own acquire.  (hipEventReleaseToDevice was measured too: no different from the default.  DESIGN 4.1 "The gap", profiles/writethrough_outputs.json)
        hipEvent_t ev = nullptr;
        if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming | hipEventDisableSystemFence)) != hipSuccess) return hip_fail(e, "hipEventCreateWithFlags");
        hipStream_t s = nullptr;
        if ((e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess) {
            (void)hipEventDestroy(ev);
            return hip_fail(e, "hipStreamCreateWithFlags");
        }
        l.max_grid = 4 * kProofWavesPerSimd * (cus > 0 ? cus : 1);  // 4 SIMDs per CU
        l.event = ev;
        l.stream = s;
    }
    *out = &l;
    return NASTAR_OK;
}

}  // namespace

extern "C" {

int nastar_verdict_abi(void) { return NASTAR_VERDICT_ABI; }

int nastar_solvable_proof_supported(int H, int W) { return (H == W && (W == 32 || W == 64)) ? 1 : 0; }

int nastar_solvable_proof(const float* cost, const float* start, const float* goal, const float* passable, int B, int H, int W,
                          int32_t* proved_out, int32_t* word, int32_t* counter, void* stream)
{
    if (!cost || !start || !goal || !passable || !word || !counter) return NASTAR_ERR_NULL;
    if (B < 1 || H < 1 || W < 1) return NASTAR_ERR_BAD_SHAPE;
    if (!nastar_solvable_proof_supported(H, W)) return NASTAR_ERR_UNSUPPORTED;
    if (!aligned16(cost) || !aligned16(start) || !aligned16(goal) || !aligned16(passable)) return NASTAR_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lock(g_lanes_mutex);
    ProofLane* l = nullptr;
    int rc = proof_lane(&l);
    if (rc) return rc;
    hipError_t e = hipEventRecord(l->event, reinterpret_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "hipEventRecord");
    if ((e = hipStreamWaitEvent(l->stream, l->event, 0)) != hipSuccess) return hip_fail(e, "hipStreamWaitEvent");
    const int mpw = 64 / W, ngroups = (B + mpw - 1) / mpw;
    const unsigned grid = (unsigned)(ngroups < l->max_grid ? ngroups : l->max_grid);
    if (W == 32) return launch(nastar_solvable_proof_kernel<5>, (int)grid, 0, l->stream, cost, start, goal, passable, B, proved_out, word, counter);
    return launch(nastar_solvable_proof_kernel<6>, (int)grid, 0, l->stream, cost, start, goal, passable, B, proved_out, word, counter);
}

int nastar_solvable_proof_sync(void)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
    if (dev < 0 || dev >= kMaxDevices) return NASTAR_OK;
    hipStream_t s = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_lanes_mutex);
        s = g_lanes[dev].stream;
    }
    if (s == nullptr) return NASTAR_OK;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    return NASTAR_OK;
}

}  // extern "C"
