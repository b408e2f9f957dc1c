// field_routes_refusals.cpp -- a stand-alone host program over csrc/nastar_field_routes_capi.hip for a sanitizer build: it calls only what
// that translation unit does BEFORE any HIP call (the argument refusals of the entry point, the limits and the workspace-size function),
// so it needs no GPU.  Build and run, from neural-astar_amd/csrc:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -o build/field_routes_refusals nastar_field_routes_capi.hip ../../tools/field_routes_refusals.cpp && build/field_routes_refusals
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../include/nastar_field_routes.h"

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
    const size_t big = (size_t)1 << 40;

    EXPECT(nastar_field_routes_abi(), 1);
    EXPECT(nastar_field_routes_max_cells(), 1179648);
    const int lds = nastar_field_routes_lds_cells();
    EXPECT(lds >= 16384 && lds <= 160 * 1024, 1);
    EXPECT(nastar_field_routes_workspace_bytes(1, 128, 128), 0);                        // the table lives in LDS
    EXPECT(nastar_field_routes_workspace_bytes(5, 1, lds), 0);
    EXPECT(nastar_field_routes_workspace_bytes(3, 1, lds + 1), (3ll * (lds + 1) + 15) / 16 * 16);
    EXPECT(nastar_field_routes_workspace_bytes(2048, 1024, 1024), 1ll << 31);           // size_t throughout
    EXPECT(nastar_field_routes_workspace_bytes(1, 1024, 1152), 1179648);
    EXPECT(nastar_field_routes_workspace_bytes(0, 512, 512), 0);
    EXPECT(nastar_field_routes_workspace_bytes(1, 1024, 1153), 0);
    EXPECT(nastar_field_routes_workspace_bytes(1, 2147483647, 2147483647), 0);
    EXPECT(nastar_field_routes_workspace_bytes(-1, -1, -1), 0);

#define ROUTES(dist, start, B, S, H, W, mask, rows, cap, len, st, ws, bytes) \
    nastar_field_routes(dist, p, p, start, B, S, H, W, mask, rows, cap, len, nullptr, st, ws, bytes, nullptr)
    EXPECT(ROUTES(nullptr, q, 2, 5, 512, 512, 0x010u, q, 16, q, q, w, big), NASTAR_ERR_UNSUPPORTED);    // the mask first
    EXPECT(ROUTES(p, q, 2, 5, 512, 512, 0x200u, q, 16, q, q, w, big), NASTAR_ERR_UNSUPPORTED);
    EXPECT(ROUTES(nullptr, q, 0, 5, 512, 512, 0x1EFu, q, 16, q, q, w, big), NASTAR_ERR_NULL);           // a NULL before the shape
    EXPECT(ROUTES(p, nullptr, 2, 5, 512, 512, 0x1EFu, q, 16, q, q, w, big), NASTAR_ERR_NULL);
    EXPECT(ROUTES(p, q, 2, 5, 512, 512, 0x1EFu, q, 16, nullptr, q, w, big), NASTAR_ERR_NULL);
    EXPECT(ROUTES(p, q, 2, 5, 512, 512, 0x1EFu, q, 16, q, nullptr, w, big), NASTAR_ERR_NULL);
    EXPECT(nastar_field_routes(p, nullptr, p, q, 2, 5, 512, 512, 0x1EFu, q, 16, q, p, q, w, big, nullptr), NASTAR_ERR_NULL);
    EXPECT(nastar_field_routes(p, p, nullptr, q, 2, 5, 512, 512, 0x1EFu, q, 16, q, p, q, w, big, nullptr), NASTAR_ERR_NULL);
    EXPECT(ROUTES(p, q, 0, 5, 1024, 1153, 0x1EFu, q, 16, q, q, w, big), NASTAR_ERR_BAD_SHAPE);          // the shape before the limit
    EXPECT(ROUTES(p, q, 2, 0, 512, 512, 0x1EFu, q, 16, q, q, w, big), NASTAR_ERR_BAD_SHAPE);
    EXPECT(ROUTES(p, q, 2, 5, -1, 512, 0x1EFu, q, 16, q, q, w, big), NASTAR_ERR_BAD_SHAPE);
    EXPECT(ROUTES(p, q, 2, 5, 512, 0, 0x1EFu, q, 16, q, q, w, big), NASTAR_ERR_BAD_SHAPE);
    EXPECT(ROUTES(p, q, 2, 5, 512, 512, 0x1EFu, q, 0, q, q, w, big), NASTAR_ERR_BAD_SHAPE);             // rows without room
    EXPECT(ROUTES(p, q, 2, 5, 512, 512, 0x1EFu, q, -3, q, q, w, big), NASTAR_ERR_BAD_SHAPE);
    EXPECT(ROUTES(p, q, 1, 5, 1024, 1153, 0x1EFu, q, 16, q, q, w, 0), NASTAR_ERR_UNSUPPORTED);          // the limit before the workspace
    EXPECT(ROUTES(p, q, 1, 5, 2147483647, 2147483647, 0x1EFu, q, 16, q, q, w, big), NASTAR_ERR_UNSUPPORTED);
    EXPECT(ROUTES(p, q, 1 << 20, (1 << 10) + 1, 8, 8, 0x1EFu, q, 16, q, q, w, big), NASTAR_ERR_UNSUPPORTED);   // more than 2^30 queries
    EXPECT(ROUTES(p, q, 2147483647, 2147483647, 8, 8, 0x1EFu, q, 16, q, q, w, big), NASTAR_ERR_UNSUPPORTED);
    EXPECT(ROUTES(p, q, 2, 5, 512, 512, 0x1EFu, q, 16, q, q, w, 0), NASTAR_ERR_WORKSPACE);
    EXPECT(ROUTES(p, q, 2, 5, 512, 512, 0x1EFu, q, 16, q, q, w, nastar_field_routes_workspace_bytes(2, 512, 512) - 1), NASTAR_ERR_WORKSPACE);
    EXPECT(ROUTES(p, q, 2, 5, 512, 512, 0x1EFu, q, 16, q, q, nullptr, big), NASTAR_ERR_WORKSPACE);
    EXPECT(ROUTES(p, q, 2, 5, 512, 512, 0x1EFu, nullptr, 0, q, q, w, 0), NASTAR_ERR_WORKSPACE);         // without rows the capacity is not looked at

    EXPECT(nastar::g_last_error[0], 0);
    printf(failures ? "%d refusal check(s) failed\n" : "all refusal checks passed (%d failures)\n", failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
