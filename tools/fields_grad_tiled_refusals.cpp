// fields_grad_tiled_refusals.cpp -- a stand-alone host program over csrc/nastar_fields_grad_tiled_capi.hip for a sanitizer build: it calls
// only what that translation unit does BEFORE any HIP call (the argument refusals of both entry points and the workspace-size function),
// so it needs no GPU.  Build and run, from neural-astar_amd/csrc:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -o build/fields_grad_tiled_refusals nastar_fields_grad_tiled_capi.hip ../../tools/fields_grad_tiled_refusals.cpp && build/fields_grad_tiled_refusals
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../include/nastar_fields_grad_tiled.h"

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
    void* w = reinterpret_cast<void*>(0x10000);
    void* odd4 = reinterpret_cast<void*>(0x10004);
    const size_t big = (size_t)1 << 40;
    int rounds = -1;

    EXPECT(nastar_fields_grad_tiled_abi(), 1);
    EXPECT(nastar_fields_grad_tiled_max_cells(), 1179648);
    EXPECT(nastar_fields_backward_tiled_workspace_bytes(1, 64, 64), (4096 * 9 + 16 + 8 + 15) / 16 * 16);
    EXPECT(nastar_fields_backward_tiled_workspace_bytes(2048, 1024, 1024), 2048ll * (1024 * 1024 * 9 + 16 + 256 * 8));
    EXPECT(nastar_fields_backward_tiled_workspace_bytes(0, 8, 8), 0);
    EXPECT(nastar_fields_backward_tiled_workspace_bytes(1, 1024, 1153), 0);
    EXPECT(nastar_fields_backward_tiled_workspace_bytes(1, 2147483647, 2147483647), 0);
    EXPECT(nastar_fields_backward_tiled_workspace_bytes(1 << 23, 70, 130), 0);
    EXPECT(nastar_fields_backward_tiled_workspace_bytes(-1, -1, -1), 0);

#define BACKWARD(dist, gd, B, H, W, mask, gc, st, ws, bytes, mr) \
    nastar_fields_backward_tiled(dist, p, p, gd, B, H, W, mask, gc, st, nullptr, ws, bytes, mr, &rounds, nullptr)
    EXPECT(BACKWARD(nullptr, p, 2, 70, 130, 0x010u, p, q, w, big, 0), NASTAR_ERR_UNSUPPORTED);   // the mask first
    EXPECT(BACKWARD(p, p, 2, 70, 130, 0x200u, p, q, w, big, 0), NASTAR_ERR_UNSUPPORTED);
    EXPECT(BACKWARD(nullptr, p, 0, 70, 130, 0x1EFu, p, q, w, big, 0), NASTAR_ERR_NULL);          // a NULL before the shape
    EXPECT(BACKWARD(p, nullptr, 2, 70, 130, 0x1EFu, p, q, w, big, 0), NASTAR_ERR_NULL);
    EXPECT(BACKWARD(p, p, 2, 70, 130, 0x1EFu, nullptr, q, w, big, 0), NASTAR_ERR_NULL);
    EXPECT(BACKWARD(p, p, 2, 70, 130, 0x1EFu, p, nullptr, w, big, 0), NASTAR_ERR_NULL);
    EXPECT(BACKWARD(p, p, 2, 70, 130, 0x1EFu, p, q, nullptr, big, 0), NASTAR_ERR_NULL);
    EXPECT(BACKWARD(p, p, 0, 1024, 1153, 0x1EFu, p, q, w, big, 0), NASTAR_ERR_BAD_SHAPE);        // the shape before the limit
    EXPECT(BACKWARD(p, p, 2, -1, 130, 0x1EFu, p, q, w, big, 0), NASTAR_ERR_BAD_SHAPE);
    EXPECT(BACKWARD(p, p, 2, 70, 130, 0x1EFu, p, q, w, big, -1), NASTAR_ERR_BAD_SHAPE);
    EXPECT(BACKWARD(p, p, 1, 1024, 1153, 0x1EFu, p, q, w, 0, 0), NASTAR_ERR_UNSUPPORTED);        // the limit before the workspace
    EXPECT(BACKWARD(p, p, 1, 2147483647, 2147483647, 0x1EFu, p, q, w, big, 0), NASTAR_ERR_UNSUPPORTED);
    EXPECT(BACKWARD(p, p, 1 << 23, 70, 130, 0x1EFu, p, q, w, big, 0), NASTAR_ERR_UNSUPPORTED);   // more than 2^24 tiles
    EXPECT(BACKWARD(p, p, 2, 70, 130, 0x1EFu, p, q, w, 0, 0), NASTAR_ERR_WORKSPACE);
    EXPECT(BACKWARD(p, p, 2, 70, 130, 0x1EFu, p, q, w, nastar_fields_backward_tiled_workspace_bytes(2, 70, 130) - 1, 0), NASTAR_ERR_WORKSPACE);
    EXPECT(BACKWARD(p, p, 2, 70, 130, 0x1EFu, p, q, odd4, big, 0), NASTAR_ERR_WORKSPACE);        // off an 8-byte boundary
    EXPECT(rounds, -1);

#define STATUS(dist, B, H, W, mask, st, ws, bytes) nastar_fields_backward_tiled_status(dist, p, p, B, H, W, mask, st, ws, bytes, nullptr)
    EXPECT(STATUS(nullptr, 2, 70, 130, 0x1FFu, q, w, big), NASTAR_ERR_UNSUPPORTED);
    EXPECT(STATUS(nullptr, 0, 70, 130, 0x1EFu, q, w, big), NASTAR_ERR_NULL);
    EXPECT(STATUS(p, 2, 70, 130, 0x1EFu, nullptr, w, big), NASTAR_ERR_NULL);
    EXPECT(STATUS(p, 2, 70, 130, 0x1EFu, q, nullptr, big), NASTAR_ERR_NULL);
    EXPECT(STATUS(p, 2, 70, 0, 0x1EFu, q, w, big), NASTAR_ERR_BAD_SHAPE);
    EXPECT(STATUS(p, 1, 1024, 1153, 0x1EFu, q, w, 0), NASTAR_ERR_UNSUPPORTED);
    EXPECT(STATUS(p, 2, 70, 130, 0x1EFu, q, w, 15), NASTAR_ERR_WORKSPACE);
    EXPECT(STATUS(p, 2, 70, 130, 0x1EFu, q, odd4, big), NASTAR_ERR_WORKSPACE);

    EXPECT(nastar::g_last_error[0], 0);
    printf(failures ? "%d refusal check(s) failed\n" : "all refusal checks passed (%d failures)\n", failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
