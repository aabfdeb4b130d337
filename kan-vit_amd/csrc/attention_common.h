// Shared between the attention translation units (attention.hip: tile forms 1-4 and the host entry points; attention16.hip:
// the 16-row-tile kernels of round 4).
#pragma once
#include "kanvit_common.h"

struct AttnArgs {
    const float* q;
    const float* k;
    const float* v;
    const float* o;
    const float* lse_in;
    const float* d_o;
    const float* delta_in;
    float* out;
    float* lse;
    float* dq;
    float* dk;
    float* dv;
    float* delta;
    float* ds;        // [B*H][NP][NP] dS = P*scale*(dP - delta), written by attn_bwd_kv2_kernel<.., DSOUT>, read by attn_bwd_dq_kernel
    long long qsb, qsh, qsn, ksb, ksh, ksn, vsb, vsh, vsn, osb, osh, osn;
    int B, H, N, D, causal, nkt, vec;
    int third;        // backward: the third-form fp32 kernels run (host side: !AttnBwdPlan::delta)
    float scale;
};

constexpr int KV_N_CU = 256;           // MI355X
constexpr float KV_LOG2E = 1.4426950408889634f;

// ---------------------------------------------------------------------------------------------
// Host-side plan of a one-work-group launch (csrc/attention.hip).  plan_attn_fwd / plan_attn_bwd are pure functions of the
// descriptor, the KANVIT_ATTN_* switches and the alignment of the pointers: kanvit_attn_bwd_workspace and the launchers read the
// same plan, so a form that hands dS through the workspace cannot be chosen without its bytes (DESIGN.md section 4, table of forms).
// ---------------------------------------------------------------------------------------------
enum AttnFwdForm { ATTN_FWD_SMALL, ATTN_FWD_16, ATTN_FWD_16_BF16, ATTN_FWD_FOURTH, ATTN_FWD_THIRD, ATTN_FWD_SECOND, ATTN_FWD_FIRST };
enum AttnBwdForm { ATTN_BWD_SMALL, ATTN_BWD_16, ATTN_BWD_16_BF16, ATTN_BWD_KV4_DQ3, ATTN_BWD_KV3_DQ3, ATTN_BWD_KV2DS_DQ, ATTN_BWD_KV2DS_DQ_BF16,
                   ATTN_BWD_KV2_Q2, ATTN_BWD_KV_Q };
enum AttnDs { ATTN_DS_NONE, ATTN_DS_F32, ATTN_DS_BF16 };      // dS hand-off from the key-stationary kernel to the dQ kernel, and its type

struct AttnFwdPlan {
    AttnFwdForm form;
    bool bf16;            // the products run on the bf16 matrix cores (a template argument of the second and first forms)
    int nkt;              // NKT bucket of the kernel template (16-row forms: the number of 16-row tiles)
    unsigned grid;
    size_t lds;           // dynamic LDS bytes
};

struct AttnBwdPlan {
    AttnBwdForm form;
    bool bf16;
    int nkt;
    unsigned grid, grid_q;      // key-stationary kernel (or the only one), query-stationary / dQ kernel
    size_t lds, lds_q;
    bool delta;           // attn_delta_kernel runs first (every two-kernel form but the third and fourth, which form rowsum(dO*O) themselves)
    AttnDs ds;
    size_t ws_bytes;      // rowsum(dO*O) [B*H*N] rounded up to 16 bytes, then dS [B*H][NP][NP]
};

// The backward's alignment tests look at three sets of pointers (each the OR of its members; 0 = aligned, the workspace query's case)
struct AttnAlign {
    uintptr_t rows;       // q | k | v | dO | dq | dk | dv: 16 bytes for every form but kv+q
    uintptr_t o;          // 16 bytes for the 16-row, fourth and third forms (they read O rows as float4 / by LDS-DMA)
    uintptr_t lse;        // 4 bytes for the 16-row forms (dword LDS-DMA)
};

AttnFwdPlan plan_attn_fwd(const kanvit_attn_desc* d, uintptr_t align);      // align = q | k | v | o
AttnBwdPlan plan_attn_bwd(const kanvit_attn_desc* d, const AttnAlign& al);

// 16-row-tile kernels (csrc/attention16.hip): the shape side of the plan (no switch, no alignment) and unconditional launchers
constexpr int KV_ATTN16_TILES = 13;      // the most tiles of a head; the one-kernel backward and the bf16 forward are built for exactly 13 (N = 193 .. 204)
int kv_attn16_tiles(const kanvit_attn_desc* d);      // 16-row tiles of a head, 0 outside the kernels' domain (D = 64, 64 < N, <= 13 tiles, three images in the LDS, 32-bit row offsets)
size_t kv_attn16_fwd_lds(int N);
size_t kv_attn16_bwd_lds();
int kv_attn16_launch_fwd(const AttnArgs& a, const AttnFwdPlan& p, hipStream_t st);
int kv_attn16_launch_bwd(const AttnArgs& a, const AttnBwdPlan& p, hipStream_t st);
