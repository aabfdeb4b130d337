// Stand-alone host-side check of csrc/kan_edge_l1.hip for a sanitizer build (no GPU needed, nothing is launched): descriptor
// validation, the band / workspace arithmetic and every refusal path with null device pointers.  Build and run (tools/README.md):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -I include \
//         tools/edge_l1_host_check.cpp kan-vit_amd/csrc/kan_edge_l1.hip -o /tmp/edge_l1_host_check && /tmp/edge_l1_host_check
#include <stdio.h>
#include <string.h>

#include "../include/kanvit.h"

thread_local char g_kanvit_err[512] = "";      // kan_layer.hip owns it in the library

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) {                                                       \
            ++failures;                                                      \
            printf("FAILED %s:%d: %s   [%s]\n", __FILE__, __LINE__, #cond, g_kanvit_err); \
        }                                                                    \
    } while (0)

static kanvit_layer_desc qkv() {       // the efficient-KAN q|k|v launch of a ViT-B block
    kanvit_layer_desc d;
    memset(&d, 0, sizeof(d));
    d.family = KANVIT_BSPLINE;
    d.groups = 36;
    d.x_group_mod = 12;
    d.I = d.O = 64;
    d.G = 8;
    d.spline_order = 3;
    d.has_base = 1;
    d.flags = KANVIT_FLAG_UNIFORM_KNOTS | KANVIT_FLAG_SHARED_BPARAMS;
    d.M = 25216;
    d.ldx = 768;
    d.ldy = 36 * 64;
    d.bparam_stride = 64 * 12;
    return d;
}

static int fwd(const kanvit_layer_desc* d) { return kanvit_edge_l1_fwd(d, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr); }
static int bwd(const kanvit_layer_desc* d) {
    return kanvit_edge_l1_bwd(d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr);
}

int main() {
    kanvit_layer_desc d = qkv();
    EXPECT(kanvit_edge_l1_supported(&d) == 1);
    EXPECT(kanvit_edge_l1_supported(nullptr) == 0);
    EXPECT(fwd(nullptr) == KANVIT_EINVAL && bwd(nullptr) == KANVIT_EINVAL);
    // bands and workspaces: multiples of the result size, a function of M alone, bounded
    for (long long M : {0LL, 1LL, 63LL, 64LL, 65LL, 256LL, 257LL, 1100LL, 25216LL, 1LL << 22, 1LL << 40}) {
        d = qkv();
        d.M = M;
        const long long bands = kanvit_edge_l1_row_bands(&d);
        EXPECT(M == 0 ? bands == 0 : (bands >= 1 && bands <= 32));
        EXPECT(kanvit_edge_l1_fwd_workspace(&d) == (size_t)bands * 4 * 36 * 64 * 64);
        EXPECT(kanvit_edge_l1_bwd_workspace(&d) == (size_t)bands * 4 * 36 * 64 * 9 * 64);
        d.groups = 12;
        EXPECT(kanvit_edge_l1_row_bands(&d) == bands);
        if (M > 0) EXPECT(fwd(&d) == KANVIT_EINVAL && strstr(g_kanvit_err, "null") && bwd(&d) == KANVIT_EINVAL);
    }
    d = qkv();
    d.M = 1100;
    EXPECT(kanvit_edge_l1_row_bands(&d) >= 3);
    // refusals by name
    struct { int family, flags; const char* word; } bad[] = {{KANVIT_SINE, 0, "SINE"}, {KANVIT_FOURIER, 0, "FOURIER"}, {KANVIT_LINEAR, 0, "LINEAR"},
                                                             {KANVIT_RBF, KANVIT_FLAG_FUSED_LN, "KANVIT_FLAG_FUSED_LN"},
                                                             {KANVIT_BSPLINE, KANVIT_FLAG_BF16_MFMA, "KANVIT_FLAG_BF16_MFMA"}};
    for (const auto& b : bad) {
        d = qkv();
        d.family = b.family;
        d.flags = b.flags;
        d.bparam_stride = 1 << 20;
        EXPECT(kanvit_edge_l1_supported(&d) == 0);
        EXPECT(kanvit_edge_l1_row_bands(&d) == 0 && kanvit_edge_l1_fwd_workspace(&d) == 0 && kanvit_edge_l1_bwd_workspace(&d) == 0);
        EXPECT(fwd(&d) == KANVIT_EINVAL && strstr(g_kanvit_err, b.word));
        EXPECT(bwd(&d) == KANVIT_EINVAL && strstr(g_kanvit_err, b.word));
    }
    // descriptor validation
    auto refused = [&](void (*edit)(kanvit_layer_desc&)) {
        kanvit_layer_desc e = qkv();
        edit(e);
        return kanvit_edge_l1_supported(&e) == 0 && fwd(&e) == KANVIT_EINVAL && bwd(&e) == KANVIT_EINVAL;
    };
    EXPECT(refused([](kanvit_layer_desc& e) { e.family = 17; }));
    EXPECT(refused([](kanvit_layer_desc& e) { e.groups = 0; }));
    EXPECT(refused([](kanvit_layer_desc& e) { e.groups = 35; }));
    EXPECT(refused([](kanvit_layer_desc& e) { e.groups = 1 << 20; e.x_group_mod = 1; }));
    EXPECT(refused([](kanvit_layer_desc& e) { e.I = 0; }));
    EXPECT(refused([](kanvit_layer_desc& e) { e.O = -3; }));
    EXPECT(refused([](kanvit_layer_desc& e) { e.M = -1; }));
    EXPECT(refused([](kanvit_layer_desc& e) { e.G = 0; }));
    EXPECT(refused([](kanvit_layer_desc& e) { e.G = 24; }));                       // 25 generated columns with the base
    EXPECT(refused([](kanvit_layer_desc& e) { e.ldx = 700; }));
    EXPECT(refused([](kanvit_layer_desc& e) { e.bparam_stride = 64 * 11; }));
    EXPECT(refused([](kanvit_layer_desc& e) { e.spline_order = -1; }));
    EXPECT(refused([](kanvit_layer_desc& e) { e.spline_order = 40; }));
    EXPECT(refused([](kanvit_layer_desc& e) { e.base_act = 6; }));
    EXPECT(refused([](kanvit_layer_desc& e) { e.has_base = 0; e.base_act = KANVIT_BASE_GELU; }));
    EXPECT(refused([](kanvit_layer_desc& e) { e.family = KANVIT_CHEBY; e.G = 5; e.has_base = 0; e.base_act = KANVIT_BASE_TANH; }));
    EXPECT(refused([](kanvit_layer_desc& e) { e.family = KANVIT_RBF; e.bparam_stride = 7; }));
    EXPECT(refused([](kanvit_layer_desc& e) { e.family = KANVIT_RBF; e.bparam_stride = 8; e.ldu = 1; }));      // [u | x] does not fit ldx
    EXPECT(refused([](kanvit_layer_desc& e) { e.family = KANVIT_RBF; e.bparam_stride = 8; e.ldu = 700; e.ldx = 4096; }));   // x block overlaps the u block
    EXPECT(refused([](kanvit_layer_desc& e) { e.family = KANVIT_RBF; e.bparam_stride = 8; e.ldu = -768; e.ldx = 4096; }));
    EXPECT(refused([](kanvit_layer_desc& e) { e.I = 1 << 20; e.O = 1 << 20; e.ldx = 1LL << 40; e.bparam_stride = 1LL << 40; }));
    d = qkv();
    d.family = KANVIT_RBF;
    d.bparam_stride = 8;
    d.ldu = 768;
    d.ldx = 1536;
    EXPECT(kanvit_edge_l1_supported(&d) == 1);
    d = qkv();
    d.family = KANVIT_CHEBY;
    d.G = 5;
    d.has_base = 0;
    d.flags = 0;
    EXPECT(kanvit_edge_l1_supported(&d) == 1 && kanvit_edge_l1_bwd_workspace(&d) == (size_t)kanvit_edge_l1_row_bands(&d) * 4 * 36 * 64 * 5 * 64);
    d = qkv();
    d.spline_order = 2;
    d.G = 9;
    d.flags = 0;
    EXPECT(kanvit_edge_l1_supported(&d) == 1);
    // the queries leave the last error alone
    d = qkv();
    d.family = KANVIT_SINE;
    fwd(&d);
    char before[512];
    memcpy(before, g_kanvit_err, sizeof(before));
    d = qkv();
    d.I = 0;
    kanvit_edge_l1_supported(&d);
    kanvit_edge_l1_row_bands(&d);
    EXPECT(memcmp(before, g_kanvit_err, sizeof(before)) == 0);
    printf(failures ? "edge_l1_host_check: %d FAILED\n" : "edge_l1_host_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
