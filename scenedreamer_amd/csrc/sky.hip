// Sky MLP for gfx950: SKYMLP.forward on PE(raydir) (imaginaire/generators/gancraft_base.py:150-169; positional encoding
// .../voxlib/positional_encoding_kernel.cu:40-75) for every ray of the frame + the frame mean (scenedreamer.py:592-598).
//
//   sky_kernel        the field MLP's layer machinery (mlp_layers.h: transposed register-resident chain, 3-term f16 split,
//                     LDS weight ring): 32 rays per wave, layers 33(->64 padded) -> 256 -> 256 x4 -> 64.  The style term
//                     fc_z_a(z) is folded into fc1's bias on the host.  The per-feature sum over rays (for sky_avg) is
//                     reduced per wave and written as one row of partial sums per wave (added up by the caller in a fixed
//                     order: reproducible, unlike float atomics).
// Its weights are packed by sky_pack_kernel and pack_mx_kernel (mlp_pack.hip).
#include "mlp_layers.h"
#include "sdn_common.h"

namespace {

constexpr int SKY_SLOTS = (4 + 4 * 16 + 4) * 4 / UNITS_PER_SLOT;   // 36
constexpr int SC_BIAS1 = 0;                                   // [256] fc1.bias + fc_z_a(z)
constexpr int SC_BIASH = 256;                                 // [4][256] fc2..fc5 bias
constexpr int SC_BC = SC_BIASH + 4 * 256;                     // [64]
constexpr int SC_TOTAL = SC_BC + 64;

struct SkyParams {
    const float *raydirs;   // [R,3] ray directions, or (PRE) [R,33] rows that are already positional-encoded
    const half8 *wpk;
    const float *consts;    // SC_TOTAL floats
    float *sky_c;           // [R,64]
    float *sky_partial;     // [4 * gridDim.x][64]: every wave's sum of sky_c over its rays (summed by the caller: no float
                            // atomics, so the frame mean is reproducible bit for bit)
    float *sky_avg;         // optional [64]: frame mean of sky_c, finished by the last workgroup to arrive
    unsigned int *counter;  // with sky_avg: arrival counter, zero before the first launch (the kernel leaves it at zero)
    int32_t R, n_tiles;
};

// element k of the positional encoding of direction d: [sin_0(3) cos_0(3) ... sin_4(3) cos_4(3) d(3)], zero padding
__device__ __forceinline__ float sky_pe(int k, float d0, float d1, float d2) {
    if (k >= SKY_IN) return 0.f;
    const int c = k % 3;
    const float x = c == 0 ? d0 : (c == 1 ? d1 : d2);
    if (k >= 30) return x;
    const int i = k / 6;
    const float rad = x * 3.141592654f * exp2f((float)i);    // positional_encoding_kernel.cu:63
    return ((k % 6) < 3) ? sinf(rad) : cosf(rad);
}

// SMX: the four hidden layers fc2..fc5 as f16 Whi.Xhi + fp6 corrections (layer8x; nothing amplifies the sky features' error)
// PRE: the input rows are SKYMLP.forward's own argument x [R,33] (the caller ran voxlib.positional_encoding, gancraft_base.py:150-157)
template <int DBG, int SMX, bool PRE = false>
__global__ __launch_bounds__(256, 1) void sky_kernel(const SkyParams p) {
    __shared__ __attribute__((aligned(1024))) char lds[LDS_TOTAL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, j = lane & 31;
    float *cst = reinterpret_cast<float *>(lds + LDS_CONST);
    for (int i = threadIdx.x; i < SC_TOTAL; i += 256) cst[i] = p.consts[i];
    __syncthreads();

    Ring r;
    r.slots_per_pass = SKY_SLOTS;
    r.wbytes = reinterpret_cast<const char *>(p.wpk);
    r.g = 0;
    r.wave = __builtin_amdgcn_readfirstlane(wave);
    r.lane = lane;
    r.voff = r.wave * (PIECES * 1024) + lane * 16;
    r.lds_lane = (unsigned)(size_t)(const lds_char *)(lds + LDS_RING) + lane * 16;
    r.src_delta = r.wave * (PIECES * 1024) - (int)(unsigned)(size_t)(const lds_char *)(lds + LDS_RING);
#pragma unroll
    for (int sl = 0; sl < DMA_AHEAD; sl++) ring_issue(lds, r, sl, sl);
    r.next_in_pass = DMA_AHEAD;

    float fsum[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};   // lane (q = j&3, h) owns features 32*ib + 8*q + 4*h + e
    const int q = j & 3;
    const int n_groups = (p.n_tiles + 3) >> 2;
    for (int grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const int tile = grp * 4 + wave;
        const int ray = tile * 32 + j;
        const bool ray_ok = tile < p.n_tiles && ray < p.R;
        const int rr = ray_ok ? ray : p.R - 1;
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
        if constexpr (!PRE) {
            d0 = p.raydirs[(size_t)rr * 3]; d1 = p.raydirs[(size_t)rr * 3 + 1]; d2 = p.raydirs[(size_t)rr * 3 + 2];
        }
        half8 bh[16], bl[16];
        f32x16 acc[8];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int k = 16 * s + 8 * h + e;
                if constexpr (PRE) v[e] = k < SKY_IN ? p.raydirs[(size_t)rr * SKY_IN + k] : 0.f;
                else v[e] = sky_pe(k, d0, d1, d2);
            }
            split8(v, bh[s], bl[s]);
        }
        float part = 0.f;
        const float *nul = cst;
        // fc1 (+ style term): 4 k-steps; fragments 0..2 of its upper half are activated behind its own lower half, the
        // remaining five (3..7) right after, the lower half behind fc2's head
        // Every layer sky_pack_kernel packs carries 2^TRUNK_SHIFT (the lo halves of weights of magnitude ~0.03 would sit in f16's
        // subnormal range otherwise: an error that is the same for every ray and so survives in the frame mean); tk takes it
        // back out in the bias fma.  The fp6 image of fc2..fc5 (pack_mx_kernel) carries no shift.
        constexpr float tk = TRUNK_K;
        layer8<DBG, 4, false, false, false>(lds, r, bh, bl, acc, cst + SC_BIAS1, cst + SC_BIAS1, nul, h, part, tk, tk);
        act_step<3, false>(acc, cst + SC_BIAS1, nul, h, bh, bl, part, tk);   // fragments 0..2 were activated inside the layer
        act_step<4, false>(acc, cst + SC_BIAS1, nul, h, bh, bl, part, tk);
        act_step<5, false>(acc, cst + SC_BIAS1, nul, h, bh, bl, part, tk);
        act_step<6, false>(acc, cst + SC_BIAS1, nul, h, bh, bl, part, tk);
        act_step<7, false>(acc, cst + SC_BIAS1, nul, h, bh, bl, part, tk);
        if constexpr (SMX) {
            // fc1's upper half (fragments 0..7 = K blocks 0, 1) was activated by the plain stages: block maxima from the
            // fragments, K block 0 converted here, K block 1 by fc2's first unit (the protocol of layer8x)
            MxState mx;
            mx.bm[2] = mx.bm[3] = 0.f;
            mx_block_max_f16<0>(bh, mx);
            mx_block_max_f16<1>(bh, mx);
            mx_convert<0>(bh, bl, mx);
#pragma unroll 1
            for (int l = 0; l < 4; l++) {
                const float *bias = cst + SC_BIASH + l * HID, *bias_pend = l == 0 ? cst + SC_BIAS1 : cst + SC_BIASH + (l - 1) * HID;
                if (l == 0) layer8x<DBG, 1, false, false>(lds, r, bh, bl, mx, acc, bias, bias_pend, nul, h, part, 1.f, tk);   // fc1's lower half is pending
                else if (l < 3) layer8x<DBG, 1, false, false>(lds, r, bh, bl, mx, acc, bias, bias_pend, nul, h, part);
                else layer8x<DBG, 2, false, false>(lds, r, bh, bl, mx, acc, bias, bias_pend, nul, h, part);
            }
        } else {
#pragma unroll 1
            for (int l = 0; l < 4; l++)
                layer8<DBG, 16, true, false, false>(lds, r, bh, bl, acc, cst + SC_BIASH + l * HID,
                                                    l == 0 ? cst + SC_BIAS1 : cst + SC_BIASH + (l - 1) * HID, nul, h, part, tk, tk);
        }
        f32x16 col[2];
        col[0] = zero16();
        col[1] = zero16();
        layer_out<DBG>(lds, r, bh, bl, acc, col, cst + SC_BIASH + 3 * HID, h, part, SMX ? 1.f : tk);
        out_descale(col, cst + SC_BC, h, tk);
        // ---- store sky_c[ray][feature] and accumulate the per-feature sum over rays -----------------------------
        if (ray_ok) {
#pragma unroll
            for (int ib = 0; ib < 2; ib++)
#pragma unroll
                for (int g4 = 0; g4 < 4; g4++)
                    *reinterpret_cast<float4 *>(p.sky_c + (size_t)ray * OUTC + 32 * ib + 8 * g4 + 4 * h) =
                        make_float4(col[ib][4 * g4], col[ib][4 * g4 + 1], col[ib][4 * g4 + 2], col[ib][4 * g4 + 3]);
        }
#pragma unroll
        for (int ib = 0; ib < 2; ib++)
#pragma unroll
            for (int rg = 0; rg < 16; rg++) {
                float v = ray_ok ? col[ib][rg] : 0.f;
                // sum over the 32 rays of this half-wave: within a row of 16 lanes by DPP (quad, half-row mirror, row mirror: every
                // lane ends up with the row's sum), ONE LDS exchange for the other row (five ds_bpermute per value before)
                v += quad_dpp<QUAD_XOR1>(v);
                v += quad_dpp<QUAD_XOR2>(v);
                v += quad_dpp<DPP_ROW_HALF_MIRROR>(v);
                v += quad_dpp<DPP_ROW_MIRROR>(v);
                v += __shfl_xor(v, 16);
                if ((rg >> 2) == q) fsum[ib][rg & 3] += v;
            }
    }
    // lanes with j < 4 (q = j) of each half hold the sums of features 32*ib + 8*q + 4*h + e
    if (j < 4) {
#pragma unroll
        for (int ib = 0; ib < 2; ib++)
#pragma unroll
            for (int e = 0; e < 4; e++)
                p.sky_partial[(size_t)(blockIdx.x * 4 + wave) * OUTC + 32 * ib + 8 * q + 4 * h + e] = fsum[ib][e];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // ---- frame mean (scenedreamer.py:592-598): the last workgroup to arrive adds the partial rows of ALL workgroups in
    //      row order (fixed order, double accumulation: reproducible bit for bit, unlike float atomics) ----------------
    if (p.sky_avg == nullptr) return;
    int *ticket = reinterpret_cast<int *>(lds + LDS_FLAGS);
    double *red = reinterpret_cast<double *>(lds + LDS_RING);      // the weight ring is idle now
    __threadfence();                                               // this workgroup's rows are visible device-wide ...
    if (threadIdx.x == 0) *ticket = (int)atomicAdd(p.counter, 1u); // ... before its arrival is counted
    __syncthreads();
    if (*ticket != (int)gridDim.x - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const int rows = 4 * (int)gridDim.x, f = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int r0 = part * (rows / 4), r1 = r0 + rows / 4;          // four consecutive quarters of the rows
    double acc_d = 0.0;
    for (int rw = r0; rw < r1; rw++) acc_d += (double)__builtin_nontemporal_load(p.sky_partial + (size_t)rw * OUTC + f);
    red[threadIdx.x] = acc_d;
    __syncthreads();
    if (threadIdx.x < OUTC) {
        const double tot = ((red[f] + red[64 + f]) + red[128 + f]) + red[192 + f];
        p.sky_avg[f] = (float)(tot / (double)p.R);
    }
    if (threadIdx.x == 0) *p.counter = 0u;                         // ready for the next launch
}

}  // namespace

extern "C" {

size_t sdn_sky_consts_floats(void) { return SC_TOTAL; }

static int sky_workgroups(int32_t n_rays, int32_t n_workgroups) {
    int wg = n_workgroups > 0 ? n_workgroups : 256;
    const int groups = sdn::div_up(sdn::div_up(n_rays, 32), 4);
    return wg > groups ? groups : wg;
}

int32_t sdn_sky_partial_rows(int32_t n_rays, int32_t n_workgroups) { return n_rays > 0 ? 4 * sky_workgroups(n_rays, n_workgroups) : 0; }

int sdn_sky_mlp(const float *raydirs, const void *packed, const float *consts, float *sky_c, float *sky_partial, int32_t n_rays,
                int32_t n_workgroups, float *sky_avg, uint32_t *counter, int32_t hidden_terms, int32_t encoded, sdn_stream_t stream) {
    SDN_REQUIRE(raydirs && packed && consts && sky_c && sky_partial && n_rays > 0, "sdn_sky_mlp: bad argument");
    SDN_REQUIRE((sky_avg == nullptr) == (counter == nullptr), "sdn_sky_mlp: sky_avg and counter go together");
    SkyParams p;
    p.sky_avg = sky_avg; p.counter = counter;
    p.raydirs = raydirs; p.wpk = (const half8 *)packed; p.consts = consts; p.sky_c = sky_c; p.sky_partial = sky_partial;
    p.R = n_rays;
    p.n_tiles = sdn::div_up(n_rays, 32);
    const int wg = sky_workgroups(n_rays, n_workgroups);
    SDN_REQUIRE(hidden_terms == 3 || hidden_terms == 6, "sdn_sky_mlp: hidden_terms must be 3 or 6");
    SDN_REQUIRE(encoded == 0 || encoded == 1, "sdn_sky_mlp: encoded must be 0 (ray directions) or 1 (positional-encoded rows)");
    if (encoded) {
        SDN_REQUIRE(hidden_terms == 3, "sdn_sky_mlp: positional-encoded input rows are evaluated with the 3-term split only");
        hipLaunchKernelGGL((sky_kernel<0, 0, true>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p);
    } else if (hidden_terms == 6) hipLaunchKernelGGL((sky_kernel<0, 1>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((sky_kernel<0, 0>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p);
    return sdn::check_launch("sdn_sky_mlp");
}

}  // extern "C"
