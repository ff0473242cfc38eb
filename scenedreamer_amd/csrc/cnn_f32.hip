// The render CNN's convolutions in plain fp32 on the f32-input matrix instruction of gfx950 (v_mfma_f32_32x32x2_f32): the
// convolutions of RenderCNN.forward (imaginaire/generators/gancraft_base.py:202-225: conv1, conv2a/2b, conv3a/3b, conv4a/4b with
// F.conv2d's zero padding, :206-219) with the epilogue of cnn.hip's conv_kernel -- bias, residual, FiLM, LeakyReLU(0.2), and
// optionally conv4 (256 -> 3) + tanh (:221, :603).  Every product is an f32 x f32 fmaf: fp32's range, no TrunkRangeError, no
// precision form to calibrate, and a summation order that is the same for every pixel wherever it lies in the frame.
//
//   conv_f32_kernel<TAPS, CIN>   (9, 256) the 3x3 layers; (1, 256) conv4a / conv4b; (1, 64) conv1.
//   pack_conv_f32_kernel         the OIHW weights in the order the kernel consumes them.
//
// Lanes, the 8-block chunk, a convolution's stream and the chunk pipeline are mlp_f32.h's (the one statement of the layout): W as
// the A operand, the 32 pixels of a wave as columns, the 256 output channels as 8 accumulator blocks.  A workgroup is 4 waves = 128
// consecutive pixels of the row-major frame; pixel p is column p & 31 of wave (p >> 5) & 3 of group p >> 7.
// Activations are plain f32 rows [H*W][C], no border: the B operand of a tap is read straight from the rows (64 B per lane and
// chunk: channels 32 b + 16 h .. + 15 of the tap's pixel, one chunk ahead of the MFMAs that use it), and a tap that falls
// outside the frame contributes 0.f -- F.conv2d(..., padding = 1).  The read always goes to an address inside the frame (clamped);
// the zero is selected when the value is used, so that no MFMA waits for more than the barrier that ends the chunk before.
// Weights: one chunk = one tap x 32 input channels x 256 outputs, TAPS * CIN / 32 per layer, multiplied by chunk_mul8_ahead.
//
// Summation order.  The MFMA is bit for bit a k-ordered fmaf chain.  One chain over the 2304 products of a 3x3 layer misses fp64
// by 6.4 - 6.8 x the error of F.conv2d in fp32 (tests/cnn_f32_ref.py); so a tap's 256 products accumulate from ZERO in a second
// accumulator set, which is then added to the running total on the VALU: taps in the order ky, kx; inside a tap the blocks b =
// 0 .. 7; inside a block k-step kk = 0 .. 15 = channels 32 b + kk, then 32 b + 16 + kk.  A 1x1 layer is one chain.
#include "mlp_f32.h"

namespace {

constexpr int COUT = 256;
constexpr int GROUP_PIXELS = 128;

struct ConvF32Params {
    const float *in;        // rows [H*W][CIN]
    const float *wpk;       // pack_conv_f32_kernel
    const float *bias;      // [256] or NULL
    const float *resid;     // rows [H*W][256] or NULL; may be `out`
    const float *mod_w;     // [256] or NULL (with mod_b)
    const float *mod_b;
    float *out;             // rows [H*W][256] or NULL
    const float *proj_w;    // [3][256] or NULL (with proj_b)
    const float *proj_b;    // [3]
    float *out_img;         // [3][H*W] tanh(raw), or NULL
    float *out_raw;         // [3][H*W], or NULL
    int32_t H, W, n_groups;
};

// The B operand of chunk (tap, blk) for this lane's pixel (y, x): 16 channels of the tap's pixel, from an address inside the frame.
// Returns whether the tap's pixel IS inside the frame (the caller selects 0.f otherwise, when it uses the values).
template <int TAPS, int CIN>
__device__ __forceinline__ bool load_b(const float *in, int H, int W, int y, int x, bool ok, int tap, int blk, int h, float4 (&v)[4]) {
    int yy = y, xx = x;
    if constexpr (TAPS == 9) {
        const int ky = tap / 3;
        yy += ky - 1;
        xx += tap - 3 * ky - 1;
    }
    const bool inside = ok && yy >= 0 && yy < H && xx >= 0 && xx < W;
    yy = yy < 0 ? 0 : (yy >= H ? H - 1 : yy);
    xx = xx < 0 ? 0 : (xx >= W ? W - 1 : xx);
    const float4 *src = reinterpret_cast<const float4 *>(in + ((size_t)yy * W + xx) * CIN + 32 * blk + 16 * h);
    v[0] = src[0]; v[1] = src[1]; v[2] = src[2]; v[3] = src[3];
    return inside;
}

__device__ __forceinline__ void select_b(const float4 (&v)[4], bool inside, float (&b)[16]) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        b[4 * i + 0] = inside ? v[i].x : 0.f;
        b[4 * i + 1] = inside ? v[i].y : 0.f;
        b[4 * i + 2] = inside ? v[i].z : 0.f;
        b[4 * i + 3] = inside ? v[i].w : 0.f;
    }
}

// the loaded values count as used HERE (and are waited for here, not later, and not touched earlier)
__device__ __forceinline__ void arrived(float4 (&bv)[4]) {
    asm volatile("" : "+v"(bv[0].x), "+v"(bv[0].y), "+v"(bv[0].z), "+v"(bv[0].w), "+v"(bv[1].x), "+v"(bv[1].y), "+v"(bv[1].z), "+v"(bv[1].w),
                      "+v"(bv[2].x), "+v"(bv[2].y), "+v"(bv[2].z), "+v"(bv[2].w), "+v"(bv[3].x), "+v"(bv[3].y), "+v"(bv[3].z), "+v"(bv[3].w));
}

// epilogue constants in LDS (f32): the per-channel vectors and conv4, so that the epilogue's only global reads are the residual's
constexpr int CST_BIAS = 0, CST_MODW = 256, CST_MODB = 512, CST_PROJW = 768, CST_PROJB = 1536, CST_TOTAL = 1540;

// this lane's pixel of group `grp`: clamped index (lanes past the end evaluate the last pixel and store nothing), row, column
struct Pixel {
    int pc, y, x;
    bool ok;
};
__device__ __forceinline__ Pixel pixel_of(int grp, int wave, int j, int HW, int W) {
    Pixel q;
    const int pix = grp * GROUP_PIXELS + wave * 32 + j;
    q.ok = pix < HW;
    q.pc = q.ok ? pix : HW - 1;
    q.y = q.pc / W;
    q.x = q.pc - q.y * W;
    return q;
}

template <int TAPS, int CIN, bool PROJ>
__global__ __launch_bounds__(256, 1) void conv_f32_kernel(const ConvF32Params p) {
    constexpr int NB = CIN / 32;                 // chunks per tap (TAPS * NB per layer); even, so a chunk's buffer is its block index & 1
    static_assert(NB % 2 == 0, "the buffer of a chunk is its index & 1");
    // two OBJECTS, so that the LDS-DMA into one is known not to alias the fragment reads from the other (field_f32.hip)
    __shared__ __attribute__((aligned(1024))) char wb0[CHUNK_BYTES];
    __shared__ __attribute__((aligned(1024))) char wb1[CHUNK_BYTES];
    __shared__ __attribute__((aligned(16))) float cst[CST_TOTAL];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31;
    const unsigned lane16 = lane * 16;
    const int HW = p.H * p.W;
    const bool has_bias = p.bias != nullptr, has_resid = p.resid != nullptr, has_mod = p.mod_w != nullptr;

    chunk_fetch(p.wpk, wb0, 0, wave, lane16);
    {
        // a term that is absent is a vector of zeros: x + 0, 0 + x and x * (0 + 1) + 0 are x (but for the sign of a zero)
        const int t = threadIdx.x;
        cst[CST_BIAS + t] = has_bias ? p.bias[t] : 0.f;
        cst[CST_MODW + t] = has_mod ? p.mod_w[t] : 0.f;
        cst[CST_MODB + t] = has_mod ? p.mod_b[t] : 0.f;
#pragma unroll
        for (int c = 0; c < 3; c++) cst[CST_PROJW + 256 * c + t] = PROJ ? p.proj_w[256 * c + t] : 0.f;
        if (t < 4) cst[CST_PROJB + t] = PROJ && t < 3 ? p.proj_b[t] : 0.f;
    }
    __syncthreads();   // from here on: at a group's start chunk 0 sits in buffer 0

    // the B operand of the chunk that comes next, always one chunk ahead: here chunk 0 of this workgroup's first group
    Pixel nq = pixel_of(blockIdx.x, wave, j, HW, p.W);
    float4 bv[4];
    bool inside = load_b<TAPS, CIN>(p.in, p.H, p.W, nq.y, nq.x, nq.ok, 0, 0, h, bv);
    arrived(bv);       // (once: inside the loop a wait for THESE loads would drain the prefetches issued after them, every group)

    for (int grp = blockIdx.x; grp < p.n_groups; grp += gridDim.x) {
        const Pixel q = pixel_of(grp, wave, j, HW, p.W);
        const int ngrp = grp + gridDim.x < p.n_groups ? grp + gridDim.x : grp;     // (after the last group: any pixel, unused)
        nq = pixel_of(ngrp, wave, j, HW, p.W);

        f32x16 tot[8];
#pragma unroll
        for (int ib = 0; ib < 8; ib++) tot[ib] = zero16();

#pragma unroll 1
        for (int tap = 0; tap < TAPS; tap++) {
            f32x16 acc[8];
            if constexpr (TAPS > 1) {
#pragma unroll
                for (int ib = 0; ib < 8; ib++) acc[ib] = zero16();
            }
#pragma unroll
            for (int blk = 0; blk < NB; blk++) {
                float b[16];
                select_b(bv, inside, b);
                // the next chunk's operands -- behind the group's last chunk: chunk 0 of this workgroup's next group
                const bool last = blk + 1 == NB && tap + 1 == TAPS;
                const int ntap = last ? 0 : (blk + 1 < NB ? tap : tap + 1), nblk = blk + 1 < NB ? blk + 1 : 0;
                inside = load_b<TAPS, CIN>(p.in, p.H, p.W, last ? nq.y : q.y, last ? nq.x : q.x, last ? nq.ok : q.ok, ntap, nblk, h, bv);
                chunk_fetch(p.wpk, (blk & 1) ? wb0 : wb1, ntap * NB + nblk, wave, lane16);
                if constexpr (TAPS > 1) chunk_mul8_ahead((blk & 1) ? wb1 : wb0, lane, b, acc);
                else chunk_mul8_ahead((blk & 1) ? wb1 : wb0, lane, b, tot);
                __syncthreads();
                // (the loaded values are not touched before the barrier: hipcc would otherwise select the zeros, or copy the
                //  registers, right behind the loads -- in the middle of this chunk's MFMAs -- and wait for them there)
                __builtin_amdgcn_sched_barrier(0);
                arrived(bv);
            }
            if constexpr (TAPS > 1) {
#pragma unroll
                for (int ib = 0; ib < 8; ib++) tot[ib] += acc[ib];
            }
        }

        // ---- epilogue, in the reference's operation order (no contraction: v * (mod_w + 1) + mod_b is a product and a sum) ----
        {
#pragma clang fp contract(off)
            const size_t row = (size_t)q.pc * COUT;
            // The residual first, a half of the channels at a time (64 registers): `resid` may be `out`, so the compiler moves no
            // read of it across a store -- read one by one, each would be a round trip to memory of its own.
            float part[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int half = 0; half < 2; half++) {
                float4 rs[4][4];
#pragma unroll
                for (int ib = 0; ib < 4; ib++)
#pragma unroll
                    for (int g = 0; g < 4; g++) rs[ib][g] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (has_resid) {
#pragma unroll
                    for (int ib = 0; ib < 4; ib++)
#pragma unroll
                        for (int g = 0; g < 4; g++) rs[ib][g] = *reinterpret_cast<const float4 *>(p.resid + row + 32 * (4 * half + ib) + 8 * g + 4 * h);
                }
#pragma unroll
                for (int ib4 = 0; ib4 < 4; ib4++)
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        const int ib = 4 * half + ib4, c0 = 32 * ib + 8 * g + 4 * h;
                        float v[4] = {tot[ib][4 * g + 0], tot[ib][4 * g + 1], tot[ib][4 * g + 2], tot[ib][4 * g + 3]};
                        const float4 bi = *reinterpret_cast<const float4 *>(cst + CST_BIAS + c0), r = rs[ib4][g];
                        const float4 s = *reinterpret_cast<const float4 *>(cst + CST_MODW + c0), t = *reinterpret_cast<const float4 *>(cst + CST_MODB + c0);
                        v[0] = r.x + (v[0] + bi.x); v[1] = r.y + (v[1] + bi.y); v[2] = r.z + (v[2] + bi.z); v[3] = r.w + (v[3] + bi.w);
                        v[0] = v[0] * (s.x + 1.f) + t.x; v[1] = v[1] * (s.y + 1.f) + t.y;
                        v[2] = v[2] * (s.z + 1.f) + t.z; v[3] = v[3] * (s.w + 1.f) + t.w;
#pragma unroll
                        for (int e = 0; e < 4; e++) v[e] = lrelu(v[e]);
                        if (p.out && q.ok) *reinterpret_cast<float4 *>(p.out + row + c0) = make_float4(v[0], v[1], v[2], v[3]);
                        if constexpr (PROJ) {   // (kept for the projection, in the accumulator's registers)
                            tot[ib][4 * g + 0] = v[0]; tot[ib][4 * g + 1] = v[1]; tot[ib][4 * g + 2] = v[2]; tot[ib][4 * g + 3] = v[3];
                        }
                    }
            }
            if constexpr (PROJ) {   // conv4 (gancraft_base.py:221) and tanh (:603): this lane's 128 channels + the other half's
#pragma unroll
                for (int ib = 0; ib < 8; ib++)
#pragma unroll
                    for (int g = 0; g < 4; g++)
#pragma unroll
                        for (int c = 0; c < 3; c++) {
                            const float4 pw = *reinterpret_cast<const float4 *>(cst + CST_PROJW + c * COUT + 32 * ib + 8 * g + 4 * h);
                            part[c] = fmaf(pw.x, tot[ib][4 * g + 0], part[c]);
                            part[c] = fmaf(pw.y, tot[ib][4 * g + 1], part[c]);
                            part[c] = fmaf(pw.z, tot[ib][4 * g + 2], part[c]);
                            part[c] = fmaf(pw.w, tot[ib][4 * g + 3], part[c]);
                        }
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float raw = part[c] + __shfl_xor(part[c], 32) + cst[CST_PROJB + c];
                    if (q.ok && h == 0) {
                        if (p.out_raw) p.out_raw[(size_t)c * HW + q.pc] = raw;
                        if (p.out_img) p.out_img[(size_t)c * HW + q.pc] = tanhf(raw);
                    }
                }
            }
        }
    }
    __syncthreads();   // (a group's last fetch -- chunk 0 for a group that never came -- lands before the LDS is released)
}

// ---- the packed stream --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_conv_f32_kernel(const float *w_oihw, int cin, int taps, float *out) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;   // one thread per float of the stream
    if (g >= (size_t)COUT * cin * taps) return;
    const int nb = cin / 32;
    const int cp = (int)(g / CHUNK_FLOATS), rem = (int)(g % CHUNK_FLOATS);
    const int tap = cp / nb, blk = cp % nb;
    const ChunkPos s = chunk_pos8(rem);
    out[g] = w_oihw[((size_t)s.row * cin + 32 * blk + 16 * s.h + s.kk) * taps + tap];
}

bool supported(int cin, int taps) { return (taps == 9 && cin == 256) || (taps == 1 && (cin == 256 || cin == 64)); }

}  // namespace

extern "C" {

size_t sdn_conv_f32_packed_weight_bytes(int cin, int taps) {
    return supported(cin, taps) ? (size_t)COUT * cin * taps * sizeof(float) : 0;
}

int sdn_conv_pack_weights_f32(const float *w_oihw, int cin, int taps, void *packed, sdn_stream_t stream) {
    if (!supported(cin, taps)) return sdn::fail(SDN_ERR_UNSUPPORTED, "sdn_conv_pack_weights_f32: unsupported (cin, taps) = (%d, %d)", cin, taps);
    SDN_REQUIRE(w_oihw && packed, "sdn_conv_pack_weights_f32: null pointer");
    const size_t n = (size_t)COUT * cin * taps;
    hipLaunchKernelGGL(pack_conv_f32_kernel, dim3((unsigned)sdn::div_up<size_t>(n, 256)), dim3(256), 0, (hipStream_t)stream, w_oihw, cin, taps,
                       (float *)packed);
    return sdn::check_launch("sdn_conv_pack_weights_f32");
}

int sdn_conv_f32(const float *in_rows, int cin, int taps, const void *packed, const float *bias, const float *resid, const float *mod_w,
                 const float *mod_b, float *out_rows, const float *proj_w, const float *proj_b, float *out_img, float *out_raw, int H, int W,
                 int n_workgroups, sdn_stream_t stream) {
    if (!supported(cin, taps)) return sdn::fail(SDN_ERR_UNSUPPORTED, "sdn_conv_f32: unsupported (cin, taps) = (%d, %d)", cin, taps);
    SDN_REQUIRE(in_rows && packed, "sdn_conv_f32: null pointer");
    SDN_REQUIRE(H > 0 && W > 0 && (int64_t)H * W <= ((int64_t)1 << 31) - GROUP_PIXELS, "sdn_conv_f32: H * W must be in [1, 2^31 - 128]");
    SDN_REQUIRE((mod_w == nullptr) == (mod_b == nullptr), "sdn_conv_f32: mod_w and mod_b go together");
    SDN_REQUIRE((proj_w == nullptr) == (proj_b == nullptr), "sdn_conv_f32: proj_w and proj_b go together");
    SDN_REQUIRE(proj_w || !(out_img || out_raw), "sdn_conv_f32: out_img / out_raw need proj_w and proj_b");
    SDN_REQUIRE(out_rows || (proj_w && (out_img || out_raw)), "sdn_conv_f32: no output");
    if (taps == 9 && out_rows == in_rows)    // a pixel's neighbours are read by other waves, at other times
        return sdn::fail(SDN_ERR_UNSUPPORTED, "sdn_conv_f32: a 3x3 layer cannot write the rows it reads (out_rows == in_rows)");
    ConvF32Params p{};
    p.in = in_rows; p.wpk = (const float *)packed; p.bias = bias; p.resid = resid; p.mod_w = mod_w; p.mod_b = mod_b;
    p.out = out_rows; p.proj_w = proj_w; p.proj_b = proj_b; p.out_img = out_img; p.out_raw = out_raw;
    p.H = H; p.W = W;
    p.n_groups = (int32_t)sdn::div_up<int64_t>((int64_t)H * W, GROUP_PIXELS);
    const int wg = n_workgroups > 0 ? n_workgroups : 256;      // persistent: one workgroup per CU
    const dim3 grid((unsigned)(wg > p.n_groups ? p.n_groups : wg));
    const hipStream_t st = (hipStream_t)stream;
    if (taps == 9) {
        if (proj_w) hipLaunchKernelGGL((conv_f32_kernel<9, 256, true>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((conv_f32_kernel<9, 256, false>), grid, dim3(256), 0, st, p);
    } else if (cin == 256) {
        if (proj_w) hipLaunchKernelGGL((conv_f32_kernel<1, 256, true>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((conv_f32_kernel<1, 256, false>), grid, dim3(256), 0, st, p);
    } else {
        if (proj_w) hipLaunchKernelGGL((conv_f32_kernel<1, 64, true>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((conv_f32_kernel<1, 64, false>), grid, dim3(256), 0, st, p);
    }
    return sdn::check_launch("sdn_conv_f32");
}

}  // extern "C"
