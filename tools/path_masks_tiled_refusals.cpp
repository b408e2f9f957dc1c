// path_masks_tiled_refusals.cpp -- a stand-alone host program over csrc/nastar_path_masks_tiled_capi.hip for a sanitizer build: it calls only
// what that translation unit does BEFORE any HIP call (the argument refusals of the two entry points, the limit and the workspace sizes),
// so it needs no GPU.  The unit calls the library's nastar_cost_to_go_tiled_workspace_bytes, so nastar_fields_tiled_capi.hip is linked
// beside it.  Build and run, from neural-astar_amd/csrc:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -o build/path_masks_tiled_refusals nastar_path_masks_tiled_capi.hip nastar_fields_tiled_capi.hip \
//         ../../tools/path_masks_tiled_refusals.cpp && build/path_masks_tiled_refusals
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../include/nastar_path_masks_tiled.h"

namespace nastar {
thread_local char g_last_error[256];  // (defined by nastar_capi.hip in the library; this program links two translation units only)
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
    void* odd = reinterpret_cast<void*>(0x10002);
    const size_t plenty = (size_t)1 << 40;
    const int limit = 1179648;

    EXPECT(nastar_path_masks_tiled_abi(), 1);
    EXPECT(nastar_path_masks_tiled_max_cells(), limit);
    EXPECT(nastar_path_masks_tiled_max_cells(), nastar_fields_tiled_max_cells());

    // the workspace sizes: 0 for what the calls refuse; the field, the relaxation's status and words; the backward adds the perturbed costs
    const int bad[][3] = {{0, 8, 8}, {-1, 8, 8}, {1, 0, 8}, {1, 8, -5}, {1, 1025, 1152}, {1, 1, limit + 1}, {1, 65536, 65536}, {1 << 24, 65, 64},
                          {2147483647, 2147483647, 2147483647}};
    for (const auto& s : bad) {
        EXPECT(nastar_path_masks_tiled_workspace_bytes(s[0], s[1], s[2]), 0);
        EXPECT(nastar_path_masks_tiled_backward_workspace_bytes(s[0], s[1], s[2]), 0);
    }
    const int good[][3] = {{1, 1, 1}, {3, 64, 64}, {2, 129, 128}, {5, 130, 259}, {1, 1024, 1152}, {2, 1, limit}, {1 << 24, 64, 64}};
    for (const auto& s : good) {
        const size_t cells4 = (size_t)s[0] * s[1] * s[2] * 4, field = nastar_cost_to_go_tiled_workspace_bytes(s[0], s[1], s[2]);
        const size_t fwd = nastar_path_masks_tiled_workspace_bytes(s[0], s[1], s[2]), back = nastar_path_masks_tiled_backward_workspace_bytes(s[0], s[1], s[2]);
        EXPECT(field > 0 && fwd >= cells4 + (size_t)s[0] * 4 + field, 1);
        EXPECT(back >= fwd + cells4, 1);
        EXPECT(fwd % 4 + back % 4, 0);
    }
    const size_t need = nastar_path_masks_tiled_workspace_bytes(2, 129, 128), need_back = nastar_path_masks_tiled_backward_workspace_bytes(2, 129, 128);

#define MASKS(cost, start, B, H, W, mask, out, st, ws, bytes, rounds) \
    nastar_path_masks_tiled(cost, p, p, start, B, H, W, mask, out, nullptr, st, ws, bytes, rounds, nullptr, nullptr)
    EXPECT(MASKS(nullptr, q, 2, 129, 128, 0x010u, p, q, p, plenty, 0), NASTAR_ERR_UNSUPPORTED);      // the mask first
    EXPECT(MASKS(p, q, 2, 129, 128, 0x200u, p, q, p, plenty, 0), NASTAR_ERR_UNSUPPORTED);
    EXPECT(MASKS(nullptr, q, 0, 129, 128, 0x1EFu, p, q, p, plenty, 0), NASTAR_ERR_NULL);             // a NULL before the shape
    EXPECT(MASKS(p, nullptr, 2, 129, 128, 0x1EFu, p, q, p, plenty, 0), NASTAR_ERR_NULL);
    EXPECT(MASKS(p, q, 2, 129, 128, 0x1EFu, nullptr, q, p, plenty, 0), NASTAR_ERR_NULL);
    EXPECT(MASKS(p, q, 2, 129, 128, 0x1EFu, p, nullptr, p, plenty, 0), NASTAR_ERR_NULL);
    EXPECT(MASKS(p, q, 2, 129, 128, 0x1EFu, p, q, nullptr, plenty, -1), NASTAR_ERR_NULL);
    EXPECT(nastar_path_masks_tiled(p, nullptr, p, q, 2, 129, 128, 0x1EFu, p, p, q, p, plenty, 0, nullptr, nullptr), NASTAR_ERR_NULL);
    EXPECT(nastar_path_masks_tiled(p, p, nullptr, q, 2, 129, 128, 0x1EFu, p, p, q, p, plenty, 0, nullptr, nullptr), NASTAR_ERR_NULL);
    EXPECT(MASKS(p, q, 0, 1025, 1152, 0x1EFu, p, q, p, plenty, 0), NASTAR_ERR_BAD_SHAPE);             // the shape before the limit
    EXPECT(MASKS(p, q, 2, -1, 128, 0x1EFu, p, q, p, plenty, 0), NASTAR_ERR_BAD_SHAPE);
    EXPECT(MASKS(p, q, 2, 129, 0, 0x1EFu, p, q, p, plenty, 0), NASTAR_ERR_BAD_SHAPE);
    EXPECT(MASKS(p, q, 2, 1025, 1152, 0x1EFu, p, q, p, plenty, -1), NASTAR_ERR_BAD_SHAPE);
    EXPECT(MASKS(p, q, 1, 1025, 1152, 0x1EFu, p, q, p, 0, 0), NASTAR_ERR_UNSUPPORTED);                // the limit before the workspace
    EXPECT(MASKS(p, q, 1, 2147483647, 2147483647, 0x1EFu, p, q, p, 0, 0), NASTAR_ERR_UNSUPPORTED);
    EXPECT(MASKS(p, q, 1 << 24, 65, 64, 0x1EFu, p, q, p, 0, 0), NASTAR_ERR_UNSUPPORTED);              // more than 2^24 tiles
    EXPECT(MASKS(p, q, 2, 129, 128, 0x1EFu, p, q, p, 0, 0), NASTAR_ERR_WORKSPACE);
    EXPECT(MASKS(p, q, 2, 129, 128, 0x1EFu, p, q, p, need - 1, 0), NASTAR_ERR_WORKSPACE);
    EXPECT(MASKS(p, q, 2, 129, 128, 0x1EFu, p, q, odd, plenty, 0), NASTAR_ERR_WORKSPACE);             // off a 4-byte boundary
    EXPECT(MASKS(p, q, 1, 1024, 1152, 0x1EFu, p, q, p, 0, 0), NASTAR_ERR_WORKSPACE);                  // AT the limit

#define BACK(cost, grad, fwd, stf, B, H, W, mask, lam, floor, out, ws, bytes, rounds) \
    nastar_path_masks_tiled_backward(cost, p, p, q, grad, fwd, stf, B, H, W, mask, lam, floor, out, nullptr, ws, bytes, rounds, nullptr, nullptr)
    const float tiny = 1e-10f;
    EXPECT(BACK(nullptr, p, p, q, 2, 129, 128, 0x010u, NAN, tiny, p, p, plenty, 0), NASTAR_ERR_UNSUPPORTED);   // the mask first
    EXPECT(BACK(nullptr, p, p, q, 0, 129, 128, 0x1EFu, 0.f, tiny, p, p, plenty, 0), NASTAR_ERR_NULL);          // a NULL before the shape and the step
    EXPECT(BACK(p, nullptr, p, q, 2, 129, 128, 0x1EFu, 20.f, tiny, p, p, plenty, 0), NASTAR_ERR_NULL);
    EXPECT(BACK(p, p, nullptr, q, 2, 129, 128, 0x1EFu, 20.f, tiny, p, p, plenty, 0), NASTAR_ERR_NULL);
    EXPECT(BACK(p, p, p, nullptr, 2, 129, 128, 0x1EFu, 20.f, tiny, p, p, plenty, 0), NASTAR_ERR_NULL);
    EXPECT(BACK(p, p, p, q, 2, 129, 128, 0x1EFu, 20.f, tiny, nullptr, p, plenty, 0), NASTAR_ERR_NULL);
    EXPECT(BACK(p, p, p, q, 2, 129, 128, 0x1EFu, 20.f, tiny, p, nullptr, plenty, 0), NASTAR_ERR_NULL);
    EXPECT(BACK(p, p, p, q, 0, 129, 128, 0x1EFu, 0.f, tiny, p, p, plenty, 0), NASTAR_ERR_BAD_SHAPE);           // the shape before the step
    EXPECT(BACK(p, p, p, q, 2, 129, 128, 0x1EFu, 0.f, tiny, p, p, plenty, -1), NASTAR_ERR_BAD_SHAPE);
    EXPECT(BACK(p, p, p, q, 2, 1025, 1152, 0x1EFu, 20.f, tiny, p, p, 0, 0), NASTAR_ERR_UNSUPPORTED);           // the limit before the workspace
    EXPECT(BACK(p, p, p, q, 2, 129, 128, 0x1EFu, 0.f, tiny, p, p, 0, 0), NASTAR_ERR_UNSUPPORTED);              // the step before the workspace
    EXPECT(BACK(p, p, p, q, 2, 129, 128, 0x1EFu, -1.f, tiny, p, p, plenty, 0), NASTAR_ERR_UNSUPPORTED);
    EXPECT(BACK(p, p, p, q, 2, 129, 128, 0x1EFu, INFINITY, tiny, p, p, plenty, 0), NASTAR_ERR_UNSUPPORTED);
    EXPECT(BACK(p, p, p, q, 2, 129, 128, 0x1EFu, NAN, tiny, p, p, plenty, 0), NASTAR_ERR_UNSUPPORTED);
    EXPECT(BACK(p, p, p, q, 2, 129, 128, 0x1EFu, 1e-45f, tiny, p, p, plenty, 0), NASTAR_ERR_UNSUPPORTED);      // a denormal: its reciprocal is not finite
    EXPECT(BACK(p, p, p, q, 2, 129, 128, 0x1EFu, 20.f, 0.f, p, p, plenty, 0), NASTAR_ERR_UNSUPPORTED);
    EXPECT(BACK(p, p, p, q, 2, 129, 128, 0x1EFu, 20.f, -0.5f, p, p, plenty, 0), NASTAR_ERR_UNSUPPORTED);
    EXPECT(BACK(p, p, p, q, 2, 129, 128, 0x1EFu, 20.f, INFINITY, p, p, plenty, 0), NASTAR_ERR_UNSUPPORTED);
    EXPECT(BACK(p, p, p, q, 2, 129, 128, 0x1EFu, 20.f, NAN, p, p, plenty, 0), NASTAR_ERR_UNSUPPORTED);
    EXPECT(BACK(p, p, p, q, 2, 129, 128, 0x1EFu, 20.f, tiny, p, p, 0, 0), NASTAR_ERR_WORKSPACE);
    EXPECT(BACK(p, p, p, q, 2, 129, 128, 0x1EFu, 20.f, tiny, p, p, need, 0), NASTAR_ERR_WORKSPACE);            // the forward's size is too small
    EXPECT(BACK(p, p, p, q, 2, 129, 128, 0x1EFu, 20.f, tiny, p, p, need_back - 1, 0), NASTAR_ERR_WORKSPACE);
    EXPECT(BACK(p, p, p, q, 2, 129, 128, 0x1EFu, 20.f, tiny, p, odd, plenty, 0), NASTAR_ERR_WORKSPACE);

    EXPECT(nastar::g_last_error[0], 0);
    printf(failures ? "%d refusal check(s) failed\n" : "all refusal checks passed (%d failures)\n", failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
