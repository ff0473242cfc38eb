// What the field kernels do around their MLP, once: the LDS prologue, the volume rendering of mc_utils.volum_rendering_relu
// (mc_utils.py:154-161) over the quad of lanes that holds a ray's 4 samples of a pass, and Generator._forward_perpix's sky
// compositing (scenedreamer.py:373-413), plus the launch helpers of their entry points (LightningMLP's (sigma, c) row store,
// store_colour_row, is mlp_layers.h's: the fp32 sky kernel stores its rows with it too).
// Shared by the f16-split kernels (field.hip: mlp_kernel, every mode) and the fp32 kernel (field_f32.hip), which
// differ in how a pass computes (sigma, col) and in nothing else: both leave sigma per lane (sample j = lane & 31, both lane
// halves) and col[ib][r] = colour feature 32 ib + 8 (r / 4) + 4 h + r % 4 of that sample.  A lane's quad (q = lane & 3) is
// one ray.  All of it is per translation unit (anonymous namespace / static), like field_enc.h, which it sits on.
#pragma once
#include "field_enc.h"

namespace {

// ---- LDS prologue (the caller passes its own LDS pointers and ends the stage with its barrier) ----------------------------------
// The constant block.  The frame mean of the sky features arrives straight from sky_kernel (no host-side copy into the block).
// ONE writer per LDS word: two waves writing the same word without a barrier in between land in either order.
__device__ __forceinline__ void stage_consts(float *cst, const float *consts, const float *sky_avg) {
    static_assert(C_SKY_AVG + OUTC == C_TOTAL, "sky_avg is the tail of the constant block");
    for (int i = threadIdx.x; i < C_TOTAL; i += 256)
        cst[i] = (sky_avg && i >= C_SKY_AVG) ? sky_avg[i - C_SKY_AVG] : consts[i];
}

// The encode stage reads its small tables from LDS: `enc` (a copy of the parameter block `src`) gets its three table
// pointers redirected, and the camera origin from device memory where the caller holds it there
__device__ __forceinline__ void stage_enc_tables(EncParams &enc, const EncParams &src, float *e_scales, float *e_lin, uint8_t *e_lut,
                                                 const float *cam_ori_dev) {
    if (threadIdx.x < NLEV) e_scales[threadIdx.x] = src.scales[threadIdx.x];
    if (threadIdx.x < src.ns + 1) e_lin[threadIdx.x] = src.lin[threadIdx.x];
    for (int i = threadIdx.x; i < 1024; i += 256) e_lut[i] = src.lut[i];
    enc.scales = e_scales; enc.lin = e_lin; enc.lut = e_lut;
    if (cam_ori_dev) {   // (uniform: three scalar loads)
        enc.ori[0] = cam_ori_dev[0]; enc.ori[1] = cam_ori_dev[1]; enc.ori[2] = cam_ori_dev[2];
    }
}

// ---- volume rendering (mc_utils.py:154-161) over the 4 samples of each ray in this pass: the weight of this lane's sample.
//      `carry` = the ray's optical depth in front of the pass, advanced past it ------------------------------------------------------
__device__ __forceinline__ float render_weight(float sigma, float dist, int q, float &carry) {
    const float fe = fmaxf(sigma, 0.f) * dist;
    float incl = fe;
    float up = quad_dpp<QUAD_UP1>(incl);
    if (q >= 1) incl += up;
    up = quad_dpp<QUAD_UP2>(incl);
    if (q >= 2) incl += up;
    float ex = quad_dpp<QUAD_UP1>(incl);
    if (q == 0) ex = 0.f;
    const float excl = carry + ex;
    const float wgt = (1.f - __expf(-fe)) * __expf(-excl);
    carry += quad_dpp<QUAD_LAST>(incl);
    return wgt;
}

// ---- outq += the pass's weighted colours of this lane's ray: lane q of the quad owns features 32 ib + 8 q + 4 h + e -----------------
__device__ __forceinline__ void accumulate_colour(const f32x16 (&col)[2], float wgt, int q, float (&outq)[2][4]) {
#pragma unroll
    for (int ib = 0; ib < 2; ib++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float rgb = fminf(fmaxf(col[ib][r], -1.f), 1.f) + 1.f;  // scenedreamer.py:408
            float v = wgt * rgb;
            v += quad_dpp<QUAD_XOR1>(v);   // sum over the 4 samples of the ray held by this quad
            v += quad_dpp<QUAD_XOR2>(v);
            if ((r >> 2) == q) outq[ib][r & 3] += v;
        }
}

// ---- any over the ray's 4 lanes (is_gnd: one of the ray's samples lies at world x <= 1, scenedreamer.py:380-382) -------------------
__device__ __forceinline__ int quad_any(bool b) {
    int g = (int)b;
    g |= quad_dpp<QUAD_XOR1>(g);
    g |= quad_dpp<QUAD_XOR2>(g);
    return g;
}

// ---- blend the sky, store (scenedreamer.py:376, :401, :408-413).  tsum: this lane's sum of weights; flag: bit 0 sky_only, bit 1
//      nosky; sky_row / out_row: the ray's row of sky_c / of the per-ray outputs (read only where ray_ok).  AUX: the blended sky
//      features and the nosky mask are returned too, each where its pointer is set -----------------------------------------------------
template <bool AUX>
__device__ __forceinline__ void blend_sky_store(const float *cst, const float *sky_c, float *net_out, int sky_row, int out_row, bool ray_ok,
                                                float tsum, uint8_t flag, const float (&outq)[2][4], int q, int h,
                                                float *skyb_out = nullptr, uint8_t *nosky_out = nullptr) {
    tsum += quad_dpp<QUAD_XOR1>(tsum);
    tsum += quad_dpp<QUAD_XOR2>(tsum);
    const bool sky_only = flag & 1, nosky = flag & 2;
    if (sky_only) tsum = 0.f;  // scenedreamer.py:376
    const float sky_w = 1.f - tsum;
    if (ray_ok) {
#pragma unroll
        for (int ib = 0; ib < 2; ib++) {
            const int f0 = 32 * ib + 8 * q + 4 * h;   // this lane owns features f0 .. f0+3 of its ray
            const float4 sc = *reinterpret_cast<const float4 *>(sky_c + (size_t)sky_row * OUTC + f0);
            const float4 sa = *reinterpret_cast<const float4 *>(cst + C_SKY_AVG + f0);
            const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, sav[4] = {sa.x, sa.y, sa.z, sa.w};
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float sky = nosky ? (scv[e] * 0.f + sav[e]) : scv[e];          // :401, mask in {0,1}
                const float rgb_sky = fminf(fmaxf(sky, -1.f), 1.f) + 1.f;
                o[e] = (sky_only ? 0.f : outq[ib][e]) + sky_w * rgb_sky - 1.f;       // :410-413
                if constexpr (AUX) {
                    if (skyb_out) skyb_out[(size_t)out_row * OUTC + f0 + e] = sky;
                }
            }
            if constexpr (AUX) {
                if (nosky_out && ib == 0 && q == 0 && h == 0) nosky_out[out_row] = nosky ? 1 : 0;
            }
            *reinterpret_cast<float4 *>(net_out + (size_t)out_row * OUTC + f0) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

}  // namespace

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// persistent workgroups of a launch over n_tiles 8-ray tiles (a workgroup takes 4 at a time): the caller's number, else 256
static int field_workgroups(int32_t n_tiles, int32_t n_workgroups) {
    const int wg = n_workgroups > 0 ? n_workgroups : 256;
    const int groups = sdn::div_up(n_tiles, 4);
    return wg > groups ? groups : wg;
}

// the window of a launch over n_rows rows of a feature matrix (LightningMLP.forward as an op): no window at all
static RayWindow raw_window(int32_t n_rows) {
    RayWindow w{};
    w.n_src = n_rows;
    return w;
}
