// The two networks upstream of every frame in plain fp32 / fp64 with a FIXED summation order: the world encoder
// (ConditionalHashGrid.forward, imaginaire/model_utils/layers.py:40-55, with the SRTConvBlocks of :6-23) and the style MLP
// (StyleMLP.forward, imaginaire/generators/gancraft_base.py:113-126).  Their results -- global_enc [1,2], the last two coordinates
// of every hash-grid lookup, and the style code z [n,256] -- are then functions of (weights, maps, style) alone: no library picks a
// solver, and the launch shape, the process and the rank are schedules that do not reach the bits.
//
//   wenc_head_f32_kernel                      hconv_head (1 -> 8) and sconv_head (11 -> 8): 3x3, stride 2, zero padding 1, bias,
//                                             LeakyReLU(0.2); NCHW maps in, channels-last rows [Ho*Wo][16] out (h | s).  VALU.
//   wenc_conv_f32_kernel<CIN, COUT, STRIDE>   the ten 3x3 convolutions of the five SRTConvBlocks (no bias, ReLU; the block's outer
//                                             LeakyReLU after a ReLU is the identity) on v_mfma_f32_32x32x2_f32.
//   wenc_pack_f32_kernel                      OIHW weights in the order the conv kernel consumes them.
//   wenc_tail_f32_kernel                      mean over the pixels, fc1 + LeakyReLU, fc2 + tanh: one workgroup, f64.
//   style_mlp_f32_kernel                      F.normalize, five fc_layers and fc_out with LeakyReLU(0.2): one workgroup per style.
//
// Lanes of the conv kernel (mlp_f32.h's: W as the A operand, 32 pixels as the columns).  Lane l = (h = l >> 5, j = l & 31) holds
// A[i = j][k = h] and B[k = h][col j]; accumulator register r of block ib holds channel 32 ib + 8 (r / 4) + 4 h + r % 4 of column j.
// A workgroup is 4 waves = 128 consecutive OUTPUT pixels of the row-major output frame; a wave evaluates its 32 pixels for up to
// four 32-channel blocks at a time (128 accumulator + 128 tap registers at most) and passes over the blocks of a wider layer, so
// COUT = 512 is four passes, not 512 accumulators.  COUT = 16 is one block whose rows 16 .. 31 are zero weights and are not stored.
// Activations are plain f32 rows [H*W][C]; the B operand of k-step kk is channel 2 kk + h of the tap's pixel, read from the rows
// (both lane halves read the same 16 B and keep their parity).  A tap outside the frame contributes 0.f, selected when the value is
// used; the read goes to a clamped address inside the frame.  Lanes past the last pixel evaluate the last pixel and store nothing.
// The packed weights: float4 ((tap * NB + ib) * CIN / 8 + kq) * 64 + lane holds, in element e, W[32 ib + j][8 kq + 2 e + h][tap]
// (NB = blocks of 32 outputs; zero for a row >= COUT): every weight once.
//
// ORDERS (the contract; tests/world_f32_ref.py restates them):
//   conv and head layers: the products of one tap accumulate from ZERO as an fmaf chain over the input channels in ascending order
//     (the MFMA is bit for bit a k-ordered fmaf chain: k-step kk = channels 2 kk, 2 kk + 1); the nine tap sums are added in f32
//     in the order ky, kx to a total that starts at zero; the head then adds the bias in f32.  This is cnn_f32.hip's rule: one
//     chain over the 9 cin products is outside 4 x E32 at cin = 256, a chain per tap is inside it.
//   tail: per channel the P rows are added in row order in f64, divided by P in f64, rounded to f32 (`pooled`); fc1 and fc2
//     accumulate their f32 x f32 products (exact in f64) in f64 in k order from zero, round to f32, add the bias in f32; LeakyReLU
//     after fc1, tanh evaluated in f64 and rounded to f32 after fc2.
//   style: sum of squares in f64 in k order, sqrt in f64 rounded to f32, max(., 1e-12f), a correctly rounded f32 division; every
//     layer's output accumulates its products in f64 in k order from zero, adds the bias in f64 and is rounded to f32 ONCE, then
//     LeakyReLU in f32.
// No float atomics, no cross-lane reduction: nothing depends on the launch shape.
#include "mlp_f32.h"

#include <cmath>

namespace {

constexpr int WENC_GROUP_PIXELS = 128;

// ---- head ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wenc_head_f32_kernel(const float *height, const float *semantic, const float *wh, const float *bh,
                                                            const float *ws, const float *bs, float *out, int H, int W, int Ho, int Wo) {
    __shared__ float s_wh[8 * 9], s_ws[8 * 11 * 9], s_b[16];
    for (int i = threadIdx.x; i < 8 * 9; i += 256) s_wh[i] = wh[i];
    for (int i = threadIdx.x; i < 8 * 11 * 9; i += 256) s_ws[i] = ws[i];
    if (threadIdx.x < 16) s_b[threadIdx.x] = threadIdx.x < 8 ? bh[threadIdx.x] : bs[threadIdx.x - 8];
    __syncthreads();
    const int64_t n = (int64_t)Ho * Wo, HW = (int64_t)H * W;
    for (int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x; pix < n; pix += (int64_t)gridDim.x * 256) {
        const int yo = (int)(pix / Wo), xo = (int)(pix - (int64_t)yo * Wo);
        float tot[16];
#pragma unroll
        for (int o = 0; o < 16; o++) tot[o] = 0.f;
#pragma unroll 1
        for (int tap = 0; tap < 9; tap++) {
            const int ky = tap / 3, kx = tap - 3 * ky;
            int yy = 2 * yo + ky - 1, xx = 2 * xo + kx - 1;
            const bool inside = yy >= 0 && yy < H && xx >= 0 && xx < W;
            yy = yy < 0 ? 0 : (yy >= H ? H - 1 : yy);
            xx = xx < 0 ? 0 : (xx >= W ? W - 1 : xx);
            const int64_t at = (int64_t)yy * W + xx;
            const float hv = height[at];
            float sv[11];
#pragma unroll
            for (int c = 0; c < 11; c++) sv[c] = semantic[c * HW + at];
            const float x0 = inside ? hv : 0.f;
#pragma unroll
            for (int o = 0; o < 8; o++) tot[o] = tot[o] + fmaf(s_wh[o * 9 + tap], x0, 0.f);
#pragma unroll
            for (int o = 0; o < 8; o++) {
                float acc = 0.f;
#pragma unroll
                for (int c = 0; c < 11; c++) acc = fmaf(s_ws[(o * 11 + c) * 9 + tap], inside ? sv[c] : 0.f, acc);
                tot[8 + o] = tot[8 + o] + acc;
            }
        }
        float4 *dst = reinterpret_cast<float4 *>(out + pix * 16);
#pragma unroll
        for (int q = 0; q < 4; q++)
            dst[q] = make_float4(lrelu(tot[4 * q] + s_b[4 * q]), lrelu(tot[4 * q + 1] + s_b[4 * q + 1]), lrelu(tot[4 * q + 2] + s_b[4 * q + 2]),
                                 lrelu(tot[4 * q + 3] + s_b[4 * q + 3]));
    }
}

// ---- the ten convolutions ----------------------------------------------------------------------------------------------------------
struct WencConvParams {
    const float *in;      // rows [H*W][CIN]
    const float4 *wpk;    // wenc_pack_f32_kernel
    float *out;           // rows [Ho*Wo][COUT]
    int32_t H, W, Ho, Wo, n_groups;
};

template <int CIN, int COUT, int STRIDE>
__global__ __launch_bounds__(256) void wenc_conv_f32_kernel(const WencConvParams p) {
    constexpr int NB = (COUT + 31) / 32;      // blocks of 32 output channels
    constexpr int NBW = NB < 4 ? NB : 4;      // ... of one pass
    constexpr int NPASS = NB / NBW;
    constexpr int KQ = CIN / 8;               // float4 of weights per lane, block and tap: 4 k-steps = 8 input channels
    static_assert(NB % NBW == 0 && CIN % 8 == 0, "whole passes, whole float4");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, j = lane & 31;
    const int HWo = p.Ho * p.Wo;

    for (int grp = blockIdx.x; grp < p.n_groups; grp += gridDim.x) {
        const int pix = grp * WENC_GROUP_PIXELS + wave * 32 + j;
        const bool ok = pix < HWo;
        const int pc = ok ? pix : HWo - 1;
        const int yo = pc / p.Wo, xo = pc - yo * p.Wo;
#pragma unroll 1
        for (int pass = 0; pass < NPASS; pass++) {
            f32x16 tot[NBW];
#pragma unroll
            for (int ib = 0; ib < NBW; ib++) tot[ib] = zero16();
#pragma unroll 1
            for (int tap = 0; tap < 9; tap++) {
                const int ky = tap / 3, kx = tap - 3 * ky;
                int yy = yo * STRIDE + ky - 1, xx = xo * STRIDE + kx - 1;
                const bool inside = yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
                yy = yy < 0 ? 0 : (yy >= p.H ? p.H - 1 : yy);
                xx = xx < 0 ? 0 : (xx >= p.W ? p.W - 1 : xx);
                const float4 *src = reinterpret_cast<const float4 *>(p.in + ((size_t)yy * p.W + xx) * CIN);
                const float4 *wp = p.wpk + (size_t)(tap * NB + pass * NBW) * KQ * 64 + lane;
                f32x16 acc[NBW];
#pragma unroll
                for (int ib = 0; ib < NBW; ib++) acc[ib] = zero16();
#pragma unroll 2
                for (int kq = 0; kq < KQ; kq++) {
                    const float4 v0 = src[2 * kq], v1 = src[2 * kq + 1];
                    float b[4] = {h ? v0.y : v0.x, h ? v0.w : v0.z, h ? v1.y : v1.x, h ? v1.w : v1.z};
#pragma unroll
                    for (int e = 0; e < 4; e++) b[e] = inside ? b[e] : 0.f;
                    float4 a[NBW];
#pragma unroll
                    for (int ib = 0; ib < NBW; ib++) a[ib] = wp[(size_t)(ib * KQ + kq) * 64];
#pragma unroll
                    for (int ib = 0; ib < NBW; ib++) acc[ib] = mfma_f32(a[ib].x, b[0], acc[ib]);
#pragma unroll
                    for (int ib = 0; ib < NBW; ib++) acc[ib] = mfma_f32(a[ib].y, b[1], acc[ib]);
#pragma unroll
                    for (int ib = 0; ib < NBW; ib++) acc[ib] = mfma_f32(a[ib].z, b[2], acc[ib]);
#pragma unroll
                    for (int ib = 0; ib < NBW; ib++) acc[ib] = mfma_f32(a[ib].w, b[3], acc[ib]);
                }
#pragma unroll
                for (int ib = 0; ib < NBW; ib++) tot[ib] += acc[ib];
            }
            if (ok) {
#pragma unroll
                for (int ib = 0; ib < NBW; ib++)
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        const int c0 = 32 * (pass * NBW + ib) + 8 * g + 4 * h;
                        if (c0 < COUT) {
                            const float v0 = tot[ib][4 * g + 0], v1 = tot[ib][4 * g + 1], v2 = tot[ib][4 * g + 2], v3 = tot[ib][4 * g + 3];
                            *reinterpret_cast<float4 *>(p.out + (size_t)pc * COUT + c0) =
                                make_float4(v0 > 0.f ? v0 : 0.f, v1 > 0.f ? v1 : 0.f, v2 > 0.f ? v2 : 0.f, v3 > 0.f ? v3 : 0.f);
                        }
                    }
            }
        }
    }
}

__host__ __device__ inline int wenc_blocks(int cout) { return (cout + 31) / 32; }

__global__ __launch_bounds__(256) void wenc_pack_f32_kernel(const float *w_oihw, int cin, int cout, float *out) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;   // one thread per float of the stream
    const int nb = wenc_blocks(cout), kqn = cin / 8;
    if (g >= (size_t)9 * nb * kqn * 256) return;
    const int e = (int)(g & 3), lane = (int)((g >> 2) & 63);
    size_t r = g >> 8;
    const int kq = (int)(r % kqn);
    r /= kqn;
    const int ib = (int)(r % nb), tap = (int)(r / nb);
    const int row = 32 * ib + (lane & 31), c = 8 * kq + 2 * e + (lane >> 5);
    out[g] = row < cout ? w_oihw[((size_t)row * cin + c) * 9 + tap] : 0.f;
}

// ---- tail ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void wenc_tail_f32_kernel(const float *rows, int P, const float *fc1_w, const float *fc1_b, const float *fc2_w,
                                                            const float *fc2_b, float *pooled, float *global_enc) {
    __shared__ float s_pool[512], s_h[16];
    const int t = threadIdx.x;
    {
        double s = 0.0;
        for (int r = 0; r < P; r++) s += (double)rows[(size_t)r * 512 + t];
        const float m = (float)(s / (double)P);
        s_pool[t] = m;
        if (pooled) pooled[t] = m;
    }
    __syncthreads();
    if (t < 16) {
        double s = 0.0;
        for (int k = 0; k < 512; k++) s = fma((double)fc1_w[t * 512 + k], (double)s_pool[k], s);
        s_h[t] = lrelu((float)s + fc1_b[t]);
    }
    __syncthreads();
    if (t < 2) {
        double s = 0.0;
        for (int k = 0; k < 16; k++) s = fma((double)fc2_w[t * 16 + k], (double)s_h[k], s);
        const float v = (float)s + fc2_b[t];
        global_enc[t] = (float)tanh((double)v);
    }
}

// ---- style MLP -----------------------------------------------------------------------------------------------------------------
struct StyleParams {
    const float *style;   // [n][128]
    const float *w[6];    // fc_layers.0 [256][128], fc_layers.1-4 and fc_out [256][256]
    const float *b[6];    // [256] each
    float *z;             // [n][256]
};

__global__ __launch_bounds__(256) void style_mlp_f32_kernel(const StyleParams p) {
    __shared__ float s_x[2][256];
    const int t = threadIdx.x;
    const float *sv = p.style + (size_t)blockIdx.x * 128;
    double ss = 0.0;
    for (int k = 0; k < 128; k++) ss = fma((double)sv[k], (double)sv[k], ss);   // (every thread the same chain)
    const float denom = fmaxf((float)sqrt(ss), 1e-12f);
    if (t < 128) s_x[0][t] = __fdiv_rn(sv[t], denom);
    __syncthreads();
#pragma unroll 1
    for (int l = 0; l < 6; l++) {
        const int K = l == 0 ? 128 : 256;
        const float *w = p.w[l] + (size_t)t * K;
        const float *x = s_x[l & 1];
        double s = 0.0;
        for (int k = 0; k < K; k++) s = fma((double)w[k], (double)x[k], s);
        const float y = lrelu((float)(s + (double)p.b[l][t]));
        s_x[(l + 1) & 1][t] = y;
        if (l == 5) p.z[(size_t)blockIdx.x * 256 + t] = y;
        __syncthreads();
    }
}

// the ten (cin, cout) pairs of the five SRTConvBlocks; the stride follows: 1 for cin == cout, 2 for cout == 2 cin
bool wenc_supported(int cin, int cout) {
    return (cin == 16 || cin == 32 || cin == 64 || cin == 128 || cin == 256) && (cout == cin || cout == 2 * cin);
}

template <int CIN, int COUT, int STRIDE>
void wenc_launch(const WencConvParams &p, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL((wenc_conv_f32_kernel<CIN, COUT, STRIDE>), grid, dim3(256), 0, st, p);
}

}  // namespace

extern "C" {

size_t sdn_wenc_f32_packed_weight_bytes(int cin, int cout) {
    return wenc_supported(cin, cout) ? (size_t)9 * cin * 32 * wenc_blocks(cout) * sizeof(float) : 0;
}

int sdn_wenc_pack_weights_f32(const float *w_oihw, int cin, int cout, void *packed, sdn_stream_t stream) {
    if (!wenc_supported(cin, cout)) return sdn::fail(SDN_ERR_UNSUPPORTED, "sdn_wenc_pack_weights_f32: unsupported (cin, cout) = (%d, %d)", cin, cout);
    SDN_REQUIRE(w_oihw && packed, "sdn_wenc_pack_weights_f32: null pointer");
    const size_t n = (size_t)9 * cin * 32 * wenc_blocks(cout);
    hipLaunchKernelGGL(wenc_pack_f32_kernel, dim3((unsigned)sdn::div_up<size_t>(n, 256)), dim3(256), 0, (hipStream_t)stream, w_oihw, cin, cout,
                       (float *)packed);
    return sdn::check_launch("sdn_wenc_pack_weights_f32");
}

int sdn_wenc_head_f32(const float *height, const float *semantic, const float *wh, const float *bh, const float *ws, const float *bs,
                      float *out_rows, int H, int W, int n_workgroups, sdn_stream_t stream) {
    SDN_REQUIRE(height && semantic && wh && bh && ws && bs && out_rows, "sdn_wenc_head_f32: null pointer");
    SDN_REQUIRE(H > 0 && W > 0 && (int64_t)H * W <= ((int64_t)1 << 31) - 256, "sdn_wenc_head_f32: H * W must be in [1, 2^31 - 256]");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int64_t blocks = sdn::div_up<int64_t>((int64_t)Ho * Wo, 256);
    const int64_t wg = n_workgroups > 0 ? n_workgroups : 4096;
    hipLaunchKernelGGL(wenc_head_f32_kernel, dim3((unsigned)(wg > blocks ? blocks : wg)), dim3(256), 0, (hipStream_t)stream, height, semantic, wh,
                       bh, ws, bs, out_rows, H, W, Ho, Wo);
    return sdn::check_launch("sdn_wenc_head_f32");
}

int sdn_wenc_conv_f32(const float *in_rows, int cin, int cout, int stride, const void *packed, float *out_rows, int H, int W, int n_workgroups,
                      sdn_stream_t stream) {
    if (!wenc_supported(cin, cout) || stride != (cout == cin ? 1 : 2))
        return sdn::fail(SDN_ERR_UNSUPPORTED, "sdn_wenc_conv_f32: unsupported (cin, cout, stride) = (%d, %d, %d)", cin, cout, stride);
    SDN_REQUIRE(in_rows && packed && out_rows, "sdn_wenc_conv_f32: null pointer");
    SDN_REQUIRE(H > 0 && W > 0 && (int64_t)H * W <= ((int64_t)1 << 31) - WENC_GROUP_PIXELS, "sdn_wenc_conv_f32: H * W must be in [1, 2^31 - 128]");
    if (out_rows == in_rows)     // a pixel's neighbours are read by other waves, at other times
        return sdn::fail(SDN_ERR_UNSUPPORTED, "sdn_wenc_conv_f32: a 3x3 layer cannot write the rows it reads (out_rows == in_rows)");
    WencConvParams p{};
    p.in = in_rows; p.wpk = (const float4 *)packed; p.out = out_rows;
    p.H = H; p.W = W;
    p.Ho = stride == 2 ? (H - 1) / 2 + 1 : H;
    p.Wo = stride == 2 ? (W - 1) / 2 + 1 : W;
    p.n_groups = (int32_t)sdn::div_up<int64_t>((int64_t)p.Ho * p.Wo, WENC_GROUP_PIXELS);
    const int wg = n_workgroups > 0 ? n_workgroups : 2048;
    const dim3 grid((unsigned)(wg > p.n_groups ? p.n_groups : wg));
    const hipStream_t st = (hipStream_t)stream;
    switch (cin * 2 + (stride - 1)) {
        case 32: wenc_launch<16, 16, 1>(p, grid, st); break;
        case 33: wenc_launch<16, 32, 2>(p, grid, st); break;
        case 64: wenc_launch<32, 32, 1>(p, grid, st); break;
        case 65: wenc_launch<32, 64, 2>(p, grid, st); break;
        case 128: wenc_launch<64, 64, 1>(p, grid, st); break;
        case 129: wenc_launch<64, 128, 2>(p, grid, st); break;
        case 256: wenc_launch<128, 128, 1>(p, grid, st); break;
        case 257: wenc_launch<128, 256, 2>(p, grid, st); break;
        case 512: wenc_launch<256, 256, 1>(p, grid, st); break;
        default: wenc_launch<256, 512, 2>(p, grid, st); break;
    }
    return sdn::check_launch("sdn_wenc_conv_f32");
}

int sdn_wenc_tail_f32(const float *rows, int P, const float *fc1_w, const float *fc1_b, const float *fc2_w, const float *fc2_b, float *pooled,
                      float *global_enc, sdn_stream_t stream) {
    SDN_REQUIRE(rows && fc1_w && fc1_b && fc2_w && fc2_b && global_enc, "sdn_wenc_tail_f32: null pointer");
    SDN_REQUIRE(P >= 1, "sdn_wenc_tail_f32: P must be >= 1");
    hipLaunchKernelGGL(wenc_tail_f32_kernel, dim3(1), dim3(512), 0, (hipStream_t)stream, rows, P, fc1_w, fc1_b, fc2_w, fc2_b, pooled, global_enc);
    return sdn::check_launch("sdn_wenc_tail_f32");
}

int sdn_style_mlp_f32(const float *style, const float *const *w6_host, const float *const *b6_host, float *z, int n, sdn_stream_t stream) {
    SDN_REQUIRE(style && w6_host && b6_host && z, "sdn_style_mlp_f32: null pointer");
    SDN_REQUIRE(n >= 1, "sdn_style_mlp_f32: n must be >= 1");
    StyleParams p{};
    p.style = style; p.z = z;
    for (int i = 0; i < 6; i++) {
        SDN_REQUIRE(w6_host[i] && b6_host[i], "sdn_style_mlp_f32: null layer pointer");
        p.w[i] = w6_host[i]; p.b[i] = b6_host[i];
    }
    hipLaunchKernelGGL(style_mlp_f32_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, p);
    return sdn::check_launch("sdn_style_mlp_f32");
}

}  // extern "C"
