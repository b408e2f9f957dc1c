// path_masks_refusals.cpp -- a stand-alone host program over csrc/nastar_path_masks_capi.hip for a sanitizer build: it calls only what that
// translation unit does BEFORE any HIP call (the argument refusals of the two entry points and the limit), so it needs no GPU.  Build and
// run, from neural-astar_amd/csrc:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -o build/path_masks_refusals nastar_path_masks_capi.hip ../../tools/path_masks_refusals.cpp && build/path_masks_refusals
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../include/nastar_path_masks.h"

namespace nastar {
thread_local char g_last_error[256];  // (defined by nastar_capi.hip in the library; this program links one translation unit only)
}

static int failures = 0;
#define EXPECT(what, want)                                                              \
    do {                                                                                \
        const long long got_ = (long long)(what);                                       \
        if (got_ != (long long)(want)) {                                                \
            printf("FAIL %s: got %lld, want %lld\n", #what, got_, (long long)(want));   \
            ++failures;                                                                 \
        }                                                                               \
    } while (0)

int main()
{
    // never dereferenced: every call below is refused on its arguments
    float* p = reinterpret_cast<float*>(0x10000);
    int32_t* q = reinterpret_cast<int32_t*>(0x10000);

    EXPECT(nastar_path_masks_abi(), 1);
    EXPECT(nastar_path_masks_max_cells(), 16384);

#define MASKS(cost, start, B, H, W, mask, out, st) nastar_path_masks(cost, p, p, start, B, H, W, mask, out, nullptr, st, nullptr)
    EXPECT(MASKS(nullptr, q, 2, 32, 32, 0x010u, p, q), NASTAR_ERR_UNSUPPORTED);          // the mask first
    EXPECT(MASKS(p, q, 2, 32, 32, 0x200u, p, q), NASTAR_ERR_UNSUPPORTED);
    EXPECT(MASKS(nullptr, q, 0, 32, 32, 0x1EFu, p, q), NASTAR_ERR_NULL);                 // a NULL before the shape
    EXPECT(MASKS(p, nullptr, 2, 32, 32, 0x1EFu, p, q), NASTAR_ERR_NULL);
    EXPECT(MASKS(p, q, 2, 32, 32, 0x1EFu, nullptr, q), NASTAR_ERR_NULL);
    EXPECT(MASKS(p, q, 2, 32, 32, 0x1EFu, p, nullptr), NASTAR_ERR_NULL);
    EXPECT(nastar_path_masks(p, nullptr, p, q, 2, 32, 32, 0x1EFu, p, p, q, nullptr), NASTAR_ERR_NULL);
    EXPECT(nastar_path_masks(p, p, nullptr, q, 2, 32, 32, 0x1EFu, p, p, q, nullptr), NASTAR_ERR_NULL);
    EXPECT(MASKS(p, q, 0, 129, 128, 0x1EFu, p, q), NASTAR_ERR_BAD_SHAPE);                // the shape before the limit
    EXPECT(MASKS(p, q, 2, -1, 32, 0x1EFu, p, q), NASTAR_ERR_BAD_SHAPE);
    EXPECT(MASKS(p, q, 2, 32, 0, 0x1EFu, p, q), NASTAR_ERR_BAD_SHAPE);
    EXPECT(MASKS(p, q, 1, 129, 128, 0x1EFu, p, q), NASTAR_ERR_UNSUPPORTED);
    EXPECT(MASKS(p, q, 1, 2147483647, 2147483647, 0x1EFu, p, q), NASTAR_ERR_UNSUPPORTED);

#define BACK(cost, grad, fwd, stf, B, H, W, mask, lam, floor, out) \
    nastar_path_masks_backward(cost, p, p, q, grad, fwd, stf, B, H, W, mask, lam, floor, out, nullptr, nullptr)
    const float tiny = 1e-10f;
    EXPECT(BACK(nullptr, p, p, q, 2, 32, 32, 0x010u, NAN, tiny, p), NASTAR_ERR_UNSUPPORTED);   // the mask first
    EXPECT(BACK(nullptr, p, p, q, 0, 32, 32, 0x1EFu, 0.f, tiny, p), NASTAR_ERR_NULL);          // a NULL before the shape and the step
    EXPECT(BACK(p, nullptr, p, q, 2, 32, 32, 0x1EFu, 20.f, tiny, p), NASTAR_ERR_NULL);
    EXPECT(BACK(p, p, nullptr, q, 2, 32, 32, 0x1EFu, 20.f, tiny, p), NASTAR_ERR_NULL);
    EXPECT(BACK(p, p, p, nullptr, 2, 32, 32, 0x1EFu, 20.f, tiny, p), NASTAR_ERR_NULL);
    EXPECT(BACK(p, p, p, q, 2, 32, 32, 0x1EFu, 20.f, tiny, nullptr), NASTAR_ERR_NULL);
    EXPECT(BACK(p, p, p, q, 0, 32, 32, 0x1EFu, 0.f, tiny, p), NASTAR_ERR_BAD_SHAPE);           // the shape before the step
    EXPECT(BACK(p, p, p, q, 2, 129, 128, 0x1EFu, 20.f, tiny, p), NASTAR_ERR_UNSUPPORTED);
    EXPECT(BACK(p, p, p, q, 2, 32, 32, 0x1EFu, 0.f, tiny, p), NASTAR_ERR_UNSUPPORTED);
    EXPECT(BACK(p, p, p, q, 2, 32, 32, 0x1EFu, -1.f, tiny, p), NASTAR_ERR_UNSUPPORTED);
    EXPECT(BACK(p, p, p, q, 2, 32, 32, 0x1EFu, INFINITY, tiny, p), NASTAR_ERR_UNSUPPORTED);
    EXPECT(BACK(p, p, p, q, 2, 32, 32, 0x1EFu, NAN, tiny, p), NASTAR_ERR_UNSUPPORTED);
    EXPECT(BACK(p, p, p, q, 2, 32, 32, 0x1EFu, 1e-45f, tiny, p), NASTAR_ERR_UNSUPPORTED);      // a denormal: its reciprocal is not finite
    EXPECT(BACK(p, p, p, q, 2, 32, 32, 0x1EFu, 20.f, 0.f, p), NASTAR_ERR_UNSUPPORTED);
    EXPECT(BACK(p, p, p, q, 2, 32, 32, 0x1EFu, 20.f, -0.5f, p), NASTAR_ERR_UNSUPPORTED);
    EXPECT(BACK(p, p, p, q, 2, 32, 32, 0x1EFu, 20.f, INFINITY, p), NASTAR_ERR_UNSUPPORTED);
    EXPECT(BACK(p, p, p, q, 2, 32, 32, 0x1EFu, 20.f, NAN, p), NASTAR_ERR_UNSUPPORTED);

    EXPECT(nastar::g_last_error[0], 0);
    printf(failures ? "%d refusal check(s) failed\n" : "all refusal checks passed (%d failures)\n", failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
