// Weight packing for gfx950: every network on the MFMA layer machinery (mlp_layers.h) gets its weights as one packed stream
// of A fragments in the machinery's unit order, written once per style code or weight set.  The packers are the only users
// of the unit order (unit_coords, kmap_*), so they share this translation unit.
//
// Kernels
//   pack_kernel        the field MLP (field.hip).  Folded MLP weights (W * alpha) are split into f16 hi + f16 lo
//                      and laid out in MFMA A-fragment order, so a wave fetches one fragment as one
//                      fully coalesced 1 KiB access and no shuffles are needed anywhere.
//   pack_mx_kernel     the colour layers' part of that stream as f16 hi fragments + block-scaled fp6 fragments
//                      of Wlo and Whi (layer8x); the same for the sky MLP's hidden layers.
//   sky_pack_kernel    the sky MLP (sky.hip).
//   head_pack_kernel, chain_pack_kernel   the render CNN's 1x1 ends (cnn_ends.hip).
#include "mlp_layers.h"
#include "sdn_common.h"

namespace {

// k index that element e of lane-half h holds in k-step s of the B operand
__host__ __device__ inline int kmap_first(int s, int h, int e) { return 16 * s + 8 * h + e; }
__host__ __device__ inline int kmap_hidden(int s, int h, int e) {
    // C/D layout of v_mfma_f32_32x32x16: register r of lane-half h holds row (r&3) + 8*(r>>2) + 4*h;
    // k-step s consumes registers 8*(s&1) .. 8*(s&1)+7 of row block s>>1
    return 32 * (s >> 1) + 16 * (s & 1) + (e & 3) + 8 * (e >> 2) + 4 * h;
}

// Unit order of the packed stream.  A unit = the 4 fragments (ib,hi) (ib,lo) (ib+1,hi) (ib+1,lo) of one k-step
// for a pair of 32-row output blocks, 4 KiB; 4 consecutive units form one 16-KiB LDS ring slot.
//   8-row-block layers: the UPPER half of the outputs (row blocks 0-3) for all k-steps comes first, then the
//   lower half (4-7): unit u -> half = u / (2*NS), s = (u % (2*NS)) / 2, ib = 4*half + 2*(u & 1).
//   This order is what lets mlp_kernel hide every activation epilogue behind MFMAs (mlp_layers.h).
//   output layer (2 row blocks): unit u = k-step u.
__host__ __device__ inline void unit_coords(int nib, int ns, int u, int &s, int &ib0) {
    if (nib == 8) {
        const int half = u / (2 * ns), rem = u % (2 * ns);
        s = rem >> 1;
        ib0 = 4 * half + 2 * (rem & 1);
    } else {
        s = u;
        ib0 = 0;
    }
}

struct PackParams {
    const float *w1;      // [256,128]
    const float *wh[5];   // [256,256] each, W * alpha already folded
    const float *wc;      // [64,256]
    half8 *out;
};

__global__ __launch_bounds__(256) void pack_kernel(const PackParams p) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;  // one thread per (layer, unit, row block of the pair, lane)
    const size_t n0 = 32 * 2 * 64, nh = 64 * 2 * 64, no = 16 * 2 * 64;
    if (g >= n0 + 5 * nh + no) return;
    int layer, nib, ns, K;
    const float *W;
    size_t base, r = g;
    if (r < n0) {
        layer = 0; nib = 8; ns = 8; K = FEAT; W = p.w1; base = 0;
    } else if (r < n0 + 5 * nh) {
        r -= n0; layer = 1 + (int)(r / nh); r %= nh; nib = 8; ns = 16; K = HID; W = p.wh[layer - 1];
        base = L0_FRAGS + (size_t)(layer - 1) * LH_FRAGS;
    } else {
        r -= n0 + 5 * nh; layer = 6; nib = 2; ns = 16; K = HID; W = p.wc; base = L0_FRAGS + 5 * LH_FRAGS;
    }
    const int lane = (int)(r % 64); r /= 64;
    const int sel = (int)(r % 2);
    const int u = (int)(r / 2);
    int s, ib0;
    unit_coords(nib, ns, u, s, ib0);
    const int row = 32 * (ib0 + sel) + (lane & 31), h = lane >> 5;
    half8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const int k = layer == 0 ? kmap_first(s, h, e) : kmap_hidden(s, h, e);
        // layers 1..6 consume a' = 1.5 x + |x| = LeakyReLU_0.2(x) / 0.4 (one v_fma instead of mul + max in the
        // MLP kernel's activation), so their weights carry the factor 0.4
        // The trunk layers (fc_1 .. fc_4, whose error the density head amplifies) are stored times 2^TRUNK_SHIFT: the lo
        // part of a weight of magnitude 0.03 is ~7e-6, deep in f16's subnormal range (quantum 6e-8), which left the split
        // weight with ~20 significant bits instead of 22; scaled by 2^shift the quantum shrinks by as much.  The kernel
        // takes the factor back out in the bias fma of the activation (act_stage, stage 1) -- no extra instruction.
        const float v = W[(size_t)row * K + k] * (layer == 0 ? 1.0f : ACT_SCALE) * (layer <= 3 ? (float)(1 << TRUNK_SHIFT) : 1.0f);
        const _Float16 vh = (_Float16)v;
        hi[e] = vh;
        lo[e] = (_Float16)(v - (float)vh);
    }
    p.out[base + ((size_t)u * 4 + 2 * sel + 0) * 64 + lane] = hi;
    p.out[base + ((size_t)u * 4 + 2 * sel + 1) * 64 + lane] = lo;
}

// ---- MX variant of the packed stream: fc_5 / fc_6 (packed layers 4 and 5) in the layout of layer8x ---------------------
// fp6 e2m3 code of |v| <= 7.5 (round to nearest even; the 32 non-negative codes are contiguous in value order)
__device__ inline unsigned fp6_code(float v) {
    const float a = fminf(fabsf(v), 7.5f);
    float c;
    if (a < 2.f) c = rintf(a * 8.f);                 // 0 .. 16: subnormals and the binade [1, 2), step 1/8
    else if (a < 4.f) c = 16.f + rintf((a - 2.f) * 4.f);
    else c = 24.f + rintf((a - 4.f) * 2.f);
    const unsigned code = (unsigned)fminf(c, 31.f);
    return code | (v < 0.f ? 32u : 0u);
}

struct PackMxParams {
    const float *wh[4];   // up to 4 hidden layers' weights [256,256] (field: fc_5, fc_6 with alpha folded; sky: fc2..fc5)
    int n_layers;
    size_t base;          // fragment index of the first of those layers in the packed stream
    half8 *out;           // the packed stream (all layers already written by pack_kernel / sky_pack_kernel)
};

__global__ __launch_bounds__(256) void pack_mx_kernel(const PackMxParams p) {
#pragma clang fp contract(off)   // hi = f16(f32(W * 0.4)) in both branches: a fused multiply would break exact ties differently
    const int g = blockIdx.x * 256 + threadIdx.x;    // one thread per (layer, unit, lane)
    if (g >= p.n_layers * 64 * 64) return;
    const int lane = g % 64, u = (g / 64) % 64, layer = g / (64 * 64);
    const float *W = p.wh[layer];
    half8 *out = p.out + p.base + (size_t)layer * LH_FRAGS + (size_t)u * 4 * 64;
    const int half = u / 32, kb = (u % 32) / 8, sub = u % 8, ib0 = 4 * half, h = lane >> 5;
    if (sub < 4) {   // f16 hi fragments of k-step 4 kb + sub for the half's 4 row blocks
        const int s = 4 * kb + sub;
        for (int f = 0; f < 4; f++) {
            const int row = 32 * (ib0 + f) + (lane & 31);
            half8 hi;
            for (int e = 0; e < 8; e++) hi[e] = (_Float16)(W[(size_t)row * HID + kmap_hidden(s, h, e)] * ACT_SCALE);
            out[f * 64 + lane] = hi;
        }
        return;
    }
    const int term = (sub - 4) / 2, iba = ib0 + 2 * ((sub - 4) % 2);   // term 0: Wlo (x x6), term 1: Whi (x xl6)
    for (int rb = 0; rb < 2; rb++) {
        const int row = 32 * (iba + rb) + (lane & 31);
        float v[32], vmax = 0.f;
        for (int i = 0; i < 32; i++) {
            const float w = W[(size_t)row * HID + kmap_hidden(4 * kb + i / 8, h, i % 8)] * ACT_SCALE;
            const float hi = (float)(_Float16)w;
            v[i] = term == 0 ? w - hi : hi;
            vmax = fmaxf(vmax, fabsf(v[i]));
        }
        int e = 0;   // smallest power of two with vmax <= 7.5 * 2^e
        if (vmax > 0.f) {
            e = (int)floorf(log2f(vmax / 7.5f)) - 1;
            while (ldexpf(7.5f, e) < vmax) e++;
        }
        if (e < -126) e = -126;
        unsigned w6[6] = {0u, 0u, 0u, 0u, 0u, 0u};
        for (int i = 0; i < 32; i++) {
            const unsigned long long code = fp6_code(ldexpf(v[i], -e));
            const int bit = 6 * i, d = bit >> 5, o = bit & 31;
            w6[d] |= (unsigned)(code << o);
            if (o > 26) w6[d + 1] |= (unsigned)(code >> (32 - o));
        }
        u32x4v f0 = {w6[0], w6[1], w6[2], w6[3]}, f1 = {w6[4], w6[5], (unsigned)(127 + e), 0u};
        out[(2 * rb) * 64 + lane] = __builtin_bit_cast(half8, f0);
        out[(2 * rb + 1) * 64 + lane] = __builtin_bit_cast(half8, f1);
    }
}

// ---- sky MLP (sky.hip): fc1 (K = 33, padded to 4 k-steps) | fc2 .. fc5 | fc_out ---------------------------------------
constexpr size_t SKY_L0_FRAGS = 16 * 4 * 64;                  // 16 units
constexpr size_t SKY_PACKED_FRAGS = SKY_L0_FRAGS + 4 * LH_FRAGS + LO_FRAGS;

struct SkyPackParams {
    const float *w1;        // [256,33]
    const float *wh[4];     // [256,256]
    const float *wc;        // [64,256]
    half8 *out;
};

__global__ __launch_bounds__(256) void sky_pack_kernel(const SkyPackParams p) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t n0 = 16 * 2 * 64, nh = 64 * 2 * 64, no = 16 * 2 * 64;
    if (g >= n0 + 4 * nh + no) return;
    int layer, nib, ns, K;
    const float *W;
    size_t base, r = g;
    if (r < n0) {
        layer = 0; nib = 8; ns = 4; K = SKY_IN; W = p.w1; base = 0;
    } else if (r < n0 + 4 * nh) {
        r -= n0; layer = 1 + (int)(r / nh); r %= nh; nib = 8; ns = 16; K = HID; W = p.wh[layer - 1];
        base = SKY_L0_FRAGS + (size_t)(layer - 1) * LH_FRAGS;
    } else {
        r -= n0 + 4 * nh; layer = 5; nib = 2; ns = 16; K = HID; W = p.wc; base = SKY_L0_FRAGS + 4 * LH_FRAGS;
    }
    const int lane = (int)(r % 64); r /= 64;
    const int sel = (int)(r % 2);
    const int u = (int)(r / 2);
    int s, ib0;
    unit_coords(nib, ns, u, s, ib0);
    const int row = 32 * (ib0 + sel) + (lane & 31), h = lane >> 5;
    half8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const int k = layer == 0 ? kmap_first(s, h, e) : kmap_hidden(s, h, e);
        float v = 0.f;
        // every layer times 2^TRUNK_SHIFT (sky_kernel takes it back out): the lo halves leave f16's subnormal range
        if (k < K) v = W[(size_t)row * K + k] * (layer == 0 ? 1.0f : ACT_SCALE) * (float)(1 << TRUNK_SHIFT);
        const _Float16 vh = (_Float16)v;
        hi[e] = vh;
        lo[e] = (_Float16)(v - (float)vh);
    }
    p.out[base + ((size_t)u * 4 + 2 * sel + 0) * 64 + lane] = hi;
    p.out[base + ((size_t)u * 4 + 2 * sel + 1) * 64 + lane] = lo;
}

// ---- render CNN tail (cnn_ends.hip chain_kernel): conv4a | conv4b | conv4 --------------------------------------------
constexpr size_t CHAIN_FRAGS = 2 * LH_FRAGS + LO_FRAGS;

struct ChainPackParams {
    const float *w4a, *w4b, *w4;   // [256,256], [256,256], [3,256]
    half8 *out;
};

__global__ __launch_bounds__(256) void chain_pack_kernel(const ChainPackParams p) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;   // one thread per (layer, unit, row block of the pair, lane)
    const size_t nh = 64 * 2 * 64, no = 16 * 2 * 64;
    if (g >= 2 * nh + no) return;
    const int layer = g < nh ? 0 : g < 2 * nh ? 1 : 2;
    size_t r = g - (size_t)layer * nh;
    const float *W = layer == 0 ? p.w4a : layer == 1 ? p.w4b : p.w4;
    const size_t base = (size_t)layer * LH_FRAGS;
    const int lane = (int)(r % 64); r /= 64;
    const int sel = (int)(r % 2);
    const int u = (int)(r / 2);
    int s, ib0;
    unit_coords(layer == 2 ? 2 : 8, 16, u, s, ib0);
    const int row = 32 * (ib0 + sel) + (lane & 31), h = lane >> 5;
    half8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        // conv4b / conv4 consume a' = LeakyReLU(x) / 0.4 (act_stage); conv4a consumes y itself
        const float w = (layer == 2 && row >= 3) ? 0.f : W[(size_t)row * HID + kmap_hidden(s, h, e)];
        // times 2^TRUNK_SHIFT like the sky MLP's stream (chain_kernel descales in its bias fmas)
        const float v = w * (layer == 0 ? 1.0f : ACT_SCALE) * (float)(1 << TRUNK_SHIFT);
        const _Float16 vh = (_Float16)v;
        hi[e] = vh;
        lo[e] = (_Float16)(v - (float)vh);
    }
    p.out[base + ((size_t)u * 4 + 2 * sel + 0) * 64 + lane] = hi;
    p.out[base + ((size_t)u * 4 + 2 * sel + 1) * 64 + lane] = lo;
}

// ---- render CNN head (cnn_ends.hip head_kernel): conv1 -------------------------------------------------------------
constexpr size_t HEAD_FRAGS = (size_t)HEAD_UNITS * 4 * 64;

struct HeadPackParams {
    const float *w1;           // [256, 64]
    half8 *out;
};

__global__ __launch_bounds__(256) void head_pack_kernel(const HeadPackParams p) {
    const int g = blockIdx.x * 256 + threadIdx.x;   // one thread per (unit, row block of the pair, lane)
    if (g >= HEAD_UNITS * 2 * 64) return;
    const int lane = g % 64, sel = (g / 64) % 2, u = g / 128;
    int s, ib0;
    unit_coords(8, HEAD_NS, u, s, ib0);
    // MFMA row rho of the block = register (rho & 3) + 4 (rho >> 3) of lane half (rho >> 2) & 1  ->  channel 32 IB + 16 h + r
    const int rho = lane & 31, ib = ib0 + sel;
    const int row = 32 * ib + 16 * ((rho >> 2) & 1) + (rho & 3) + 4 * (rho >> 3);
    const int h = lane >> 5;
    half8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const float v = p.w1[(size_t)row * HEAD_K + kmap_first(s, h, e)];
        const _Float16 vh = (_Float16)v;
        hi[e] = vh;
        lo[e] = (_Float16)(v - (float)vh);
    }
    p.out[((size_t)u * 4 + 2 * sel + 0) * 64 + lane] = hi;
    p.out[((size_t)u * 4 + 2 * sel + 1) * 64 + lane] = lo;
}

}  // namespace

extern "C" {

size_t sdn_field_packed_weight_bytes(void) { return PACKED_FRAGS * sizeof(half8); }
int sdn_field_trunk_shift(void) { return TRUNK_SHIFT; }

int sdn_field_pack_weights(const float *w1, const float *const *wh5_host, const float *wc, void *packed,
                           sdn_stream_t stream) {
    SDN_REQUIRE(w1 && wh5_host && wc && packed, "sdn_field_pack_weights: null pointer");
    PackParams p;
    p.w1 = w1;
    for (int i = 0; i < 5; i++) {
        SDN_REQUIRE(wh5_host[i], "sdn_field_pack_weights: null hidden weight");
        p.wh[i] = wh5_host[i];
    }
    p.wc = wc;
    p.out = (half8 *)packed;
    const size_t n = 8 * 8 * 64 + 5 * 16 * 8 * 64 + 16 * 2 * 64;
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)sdn::div_up<size_t>(n, 256)), dim3(256), 0, (hipStream_t)stream, p);
    return sdn::check_launch("sdn_field_pack_weights");
}

int sdn_field_pack_weights_mx(const float *w1, const float *const *wh5_host, const float *wc, void *packed, sdn_stream_t stream) {
    if (int rc = sdn_field_pack_weights(w1, wh5_host, wc, packed, stream)) return rc;
    PackMxParams p;
    p.wh[0] = wh5_host[3];   // fc_5
    p.wh[1] = wh5_host[4];   // fc_6
    p.wh[2] = p.wh[3] = nullptr;
    p.n_layers = 2;
    p.base = L0_FRAGS + 3 * LH_FRAGS;
    p.out = (half8 *)packed;
    hipLaunchKernelGGL(pack_mx_kernel, dim3(2 * 64 * 64 / 256), dim3(256), 0, (hipStream_t)stream, p);
    return sdn::check_launch("sdn_field_pack_weights_mx");
}

size_t sdn_sky_packed_weight_bytes(void) { return SKY_PACKED_FRAGS * sizeof(half8); }

int sdn_sky_pack_weights(const float *w1, const float *const *wh4_host, const float *wc, void *packed, sdn_stream_t stream) {
    SDN_REQUIRE(w1 && wh4_host && wc && packed, "sdn_sky_pack_weights: null pointer");
    SkyPackParams p;
    p.w1 = w1;
    for (int i = 0; i < 4; i++) {
        SDN_REQUIRE(wh4_host[i], "sdn_sky_pack_weights: null hidden weight");
        p.wh[i] = wh4_host[i];
    }
    p.wc = wc;
    p.out = (half8 *)packed;
    const size_t n = 16 * 2 * 64 + 4 * 64 * 2 * 64 + 16 * 2 * 64;
    hipLaunchKernelGGL(sky_pack_kernel, dim3((unsigned)sdn::div_up<size_t>(n, 256)), dim3(256), 0, (hipStream_t)stream, p);
    return sdn::check_launch("sdn_sky_pack_weights");
}

int sdn_sky_pack_weights_mx(const float *w1, const float *const *wh4_host, const float *wc, void *packed, sdn_stream_t stream) {
    if (int rc = sdn_sky_pack_weights(w1, wh4_host, wc, packed, stream)) return rc;
    PackMxParams p;
    for (int i = 0; i < 4; i++) p.wh[i] = wh4_host[i];
    p.n_layers = 4;
    p.base = SKY_L0_FRAGS;
    p.out = (half8 *)packed;
    hipLaunchKernelGGL(pack_mx_kernel, dim3(4 * 64 * 64 / 256), dim3(256), 0, (hipStream_t)stream, p);
    return sdn::check_launch("sdn_sky_pack_weights_mx");
}

size_t sdn_conv_chain_packed_weight_bytes(void) { return CHAIN_FRAGS * sizeof(half8); }

int sdn_conv_chain_pack_weights(const float *w4a, const float *w4b, const float *w4, void *packed, sdn_stream_t stream) {
    SDN_REQUIRE(w4a && w4b && w4 && packed, "sdn_conv_chain_pack_weights: null pointer");
    ChainPackParams p;
    p.w4a = w4a; p.w4b = w4b; p.w4 = w4; p.out = (half8 *)packed;
    const size_t n = 2 * 64 * 2 * 64 + 16 * 2 * 64;
    hipLaunchKernelGGL(chain_pack_kernel, dim3((unsigned)sdn::div_up<size_t>(n, 256)), dim3(256), 0, (hipStream_t)stream, p);
    return sdn::check_launch("sdn_conv_chain_pack_weights");
}

size_t sdn_conv_head_packed_weight_bytes(void) { return HEAD_FRAGS * sizeof(half8); }

int sdn_conv_head_pack_weights(const float *w1, void *packed, sdn_stream_t stream) {
    SDN_REQUIRE(w1 && packed, "sdn_conv_head_pack_weights: null pointer");
    HeadPackParams p;
    p.w1 = w1; p.out = (half8 *)packed;
    hipLaunchKernelGGL(head_pack_kernel, dim3(sdn::div_up(HEAD_UNITS * 2 * 64, 256)), dim3(256), 0, (hipStream_t)stream, p);
    return sdn::check_launch("sdn_conv_head_pack_weights");
}

}  // extern "C"
