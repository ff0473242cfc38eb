// The fp32 layer code of the exact rung on the f32-input matrix instruction of gfx950 (v_mfma_f32_32x32x2_f32), shared by the field
// (field_f32.hip), the sky MLP (sky_f32.hip) and the render CNN's convolutions (cnn_f32.hip): every product is an f32 x f32 fmaf,
// the MFMA result is bit for bit a k-ordered fmaf chain.  All of it is per translation unit (anonymous namespace, force-inlined),
// like mlp_layers.h.  This comment is the one statement of the lane layout and of the packed streams; tests/f32_pack_layout.py
// restates it in numpy and tests/test_f32_pack_*.py hold the three pack kernels to it.
//
// Lanes.  A layer is evaluated transposed, W as the A operand (32 output channels per block), 32 rows (samples, rays, pixels) as
// the columns.  Lane l = (h = l >> 5, j = l & 31) holds A[i = j][k = h] and B[k = h][col j], one f32 each; accumulator register r
// of lane (h, j) holds channel 8 (r / 4) + 4 h + r % 4 of column j (kmap_f32).
//
// Streams.  A layer's weights are a sequence of chunks of 32 KiB = 8192 f32, of two kinds; a lane of a k-step is a lane of the MFMA
// that consumes it, so lane (h, j) of block ib holds W[32 ib + j][k], k = the input channel that B's lane half h carries then:
//   8-block chunk (chunk_pos8; read by chunk_mul8 / chunk_mul8_ahead): 16 k-steps x [blocks 0-3 | blocks 4-7][lane][4 blocks], i.e.
//                 float 512 kk + 256 (ib / 4) + 4 lane + ib % 4 = k-step kk, block ib: a lane reads two float4 per k-step.
//   2-block chunk (chunk_pos2; read by chunk_out2): 64 k-steps x [lane][2 blocks], float 128 kk + 2 lane + ib.
// Which k a (chunk, k-step, h) stands for is the consumer's choice of B operand:
//   hidden layer of an MLP (8 chunks): chunk b = input block b, k-step r <-> k = 32 b + kmap_f32(r, h): accumulator register r of
//                 block b, after bias + LeakyReLU, IS the B operand of that k-step.  Activations never leave the registers and never
//                 cross lanes.
//   fc_out_c (2 chunks, 64 x 256): chunk C, k-step kk <-> k = 32 (4 C + kk / 16) + kmap_f32(kk % 16, h).
//   the field's fc_1 (4 chunks, K = 128): chunk c, k-step kk <-> k = 16 (2 c + kk / 8) + 8 h + kk % 8 (hash-grid level 2 s + h, s =
//                 2 c + kk / 8, channel kk % 8: the encode stage's lane half h blends the levels 2 s + h).
//   the sky's fc1 (2 chunks, K = 33 zero-padded to 64): chunk c, k-step kk <-> k = 2 (16 c + kk) + h; zero where k >= 33.
//   a convolution (taps x cin / 32 chunks, OIHW weights): chunk tap * (cin / 32) + blk, k-step kk <-> input channel 32 blk + 16 h +
//                 kk of tap (ky, kx) = (tap / 3, tap % 3).
// The MLP streams are fc_1 | the hidden layers | fc_out_c (field: 4 + 5 x 8 + 2 = 46 chunks, sky: 2 + 4 x 8 + 2 = 36).
//
// The four waves of a workgroup share one copy: chunk n + 1 is copied L2 -> LDS (global_load_lds, 16 B per lane, lane-linear image)
// into the second buffer while chunk n is multiplied (128 MFMAs of 64 cycles per wave); one __syncthreads() per chunk ends both.
#pragma once
#include "mlp_layers.h"
#include "sdn_common.h"

namespace {

constexpr int CHUNK_BYTES = 32768;
constexpr int CHUNK_FLOATS = CHUNK_BYTES / 4;

__device__ __forceinline__ float lrelu(float x) { return x > 0.f ? x : 0.2f * x; }   // F.leaky_relu(x, 0.2)

__device__ __forceinline__ f32x16 mfma_f32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// ---- the stream layout, for the pack kernels ---------------------------------------------------------------------------------------
// channel that accumulator register r of lane half h holds inside its 32-channel block = k of k-step r of that input block
__host__ __device__ inline int kmap_f32(int r, int h) { return 8 * (r >> 2) + 4 * h + (r & 3); }

// float `rem` of a chunk: its k-step, the lane half that multiplies it, and the weight's row (output channel)
struct ChunkPos {
    int kk, h, row;
};
__host__ __device__ inline ChunkPos chunk_pos8(int rem) {
    const int in = rem % 512, ib = 4 * (in / 256) + (in & 3), lane = (in % 256) / 4;
    return {rem / 512, lane >> 5, 32 * ib + (lane & 31)};
}
__host__ __device__ inline ChunkPos chunk_pos2(int rem) {
    const int in = rem % 128, ib = in & 1, lane = in / 2;
    return {rem / 128, lane >> 5, 32 * ib + (lane & 31)};
}

// An MLP's stream: N1 chunks of its first layer | NH hidden layers | fc_out_c
template <int NH>
struct MlpPackF32 {
    const float *w1;       // the first layer, [256, K]
    const float *wh[NH];   // [256,256] each
    const float *wc;       // [64,256]
    float *out;
};

// float g of that stream; first(chunk, pos) is the first layer's, whose k-order is its kernel's
template <int N1, int NH, class First>
__device__ __forceinline__ float mlp_stream_weight(const MlpPackF32<NH> &p, size_t g, First first) {
    const int cp = (int)(g / CHUNK_FLOATS), rem = (int)(g % CHUNK_FLOATS);
    if (cp < N1 + 8 * NH) {
        const ChunkPos s = chunk_pos8(rem);
        if (cp < N1) return first(cp, s);
        return p.wh[(cp - N1) / 8][(size_t)s.row * HID + 32 * ((cp - N1) % 8) + kmap_f32(s.kk, s.h)];
    }
    const ChunkPos s = chunk_pos2(rem);
    return p.wc[(size_t)s.row * HID + 32 * (4 * (cp - (N1 + 8 * NH)) + (s.kk >> 4)) + kmap_f32(s.kk & 15, s.h)];
}

// the two MLP pack entries: argument checks, launch of `kernel` with one thread per float
template <int NH, class Kernel>
int pack_mlp_weights_f32(const char *who, Kernel kernel, size_t n_floats, const float *w1, const float *const *wh_host, const float *wc,
                         void *packed, sdn_stream_t stream) {
    if (!(w1 && wh_host && wc && packed)) return sdn::fail(SDN_ERR_INVALID, "%s: null pointer", who);
    MlpPackF32<NH> p;
    p.w1 = w1;
    for (int i = 0; i < NH; i++) {
        if (!wh_host[i]) return sdn::fail(SDN_ERR_INVALID, "%s: null hidden weight", who);
        p.wh[i] = wh_host[i];
    }
    p.wc = wc;
    p.out = (float *)packed;
    hipLaunchKernelGGL(kernel, dim3((unsigned)sdn::div_up<size_t>(n_floats, 256)), dim3(256), 0, (hipStream_t)stream, p);
    return sdn::check_launch(who);
}

// ---- chunks: L2 -> LDS, LDS -> MFMA ------------------------------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ void chunk_piece(const char *lane_src, char *dst) {
    // the immediate offset (a 13-bit signed field: below 4096) is added to the global AND to the LDS address
    __builtin_amdgcn_global_load_lds((glb_char *)(lane_src + (K / 4) * 4096), (lds_char *)(dst + (K / 4) * 4096), 16, (K % 4) * 1024, 0);
}

// this wave's quarter of chunk `cp` of the stream -> weight buffer `wbuf`: 8 pieces of 1 KiB (64 lanes x 16 B).
// The source address is a uniform base + this lane's 32-bit byte offset (the saddr form of the load): as 64-bit per-lane
// pointers hipcc hoists the 8 addresses of every call out of the pass loop and keeps them in scratch memory.
__device__ __forceinline__ void chunk_fetch(const float *wpk, char *wbuf, int cp, int wave, unsigned lane16) {
    const char *src = reinterpret_cast<const char *>(wpk) + (size_t)cp * CHUNK_BYTES + wave * 8192;    // uniform
    char *dst = wbuf + wave * 8192;      // wave-uniform; the DMA adds lane * 16
    asm volatile("" : "+v"(lane16));
    chunk_piece<0>(src + lane16, dst); chunk_piece<1>(src + lane16, dst); chunk_piece<2>(src + lane16, dst); chunk_piece<3>(src + lane16, dst);
    chunk_piece<4>(src + lane16, dst); chunk_piece<5>(src + lane16, dst); chunk_piece<6>(src + lane16, dst); chunk_piece<7>(src + lane16, dst);
}

// acc[ib] (+)= sum over 16 k-steps of W_chunk[ib][k-step] x b[k-step]: one 8-block chunk, two conflict-free float4 reads per k-step.
// TWO loops with the same products in the same order.  chunk_mul8 leaves the placing of the reads to hipcc and is what the MLP
// kernels (field_f32.hip, sky_f32.hip) were measured with; chunk_mul8_ahead reads the fragments of k-step kk + 1 while k-step kk is
// multiplied, pinned by scheduling groups (left alone, hipcc reads each float4 right in front of its four MFMAs and exposes an LDS
// round trip per four), and is what the convolution kernel (cnn_f32.hip) was measured with.  Neither kernel has been timed with
// the other's loop; replacing one by the other is a performance change of its own.
__device__ __forceinline__ void chunk_mul8(const char *wbuf, int lane, const float (&b)[16], f32x16 (&acc)[8]) {
    const float4 *w = reinterpret_cast<const float4 *>(wbuf) + lane;
#pragma unroll
    for (int kk = 0; kk < 16; kk++) {
        const float4 a0 = w[kk * 128], a1 = w[kk * 128 + 64];
        acc[0] = mfma_f32(a0.x, b[kk], acc[0]);
        acc[1] = mfma_f32(a0.y, b[kk], acc[1]);
        acc[2] = mfma_f32(a0.z, b[kk], acc[2]);
        acc[3] = mfma_f32(a0.w, b[kk], acc[3]);
        acc[4] = mfma_f32(a1.x, b[kk], acc[4]);
        acc[5] = mfma_f32(a1.y, b[kk], acc[5]);
        acc[6] = mfma_f32(a1.z, b[kk], acc[6]);
        acc[7] = mfma_f32(a1.w, b[kk], acc[7]);
    }
}

__device__ __forceinline__ void chunk_mul8_ahead(const char *wbuf, int lane, const float (&b)[16], f32x16 (&acc)[8]) {
    const float4 *w = reinterpret_cast<const float4 *>(wbuf) + lane;
    float4 a0 = w[0], a1 = w[64];
#pragma unroll
    for (int kk = 0; kk < 16; kk++) {
        float4 n0 = a0, n1 = a1;
        if (kk < 15) { n0 = w[(kk + 1) * 128]; n1 = w[(kk + 1) * 128 + 64]; }
        acc[0] = mfma_f32(a0.x, b[kk], acc[0]);
        acc[1] = mfma_f32(a0.y, b[kk], acc[1]);
        acc[2] = mfma_f32(a0.z, b[kk], acc[2]);
        acc[3] = mfma_f32(a0.w, b[kk], acc[3]);
        acc[4] = mfma_f32(a1.x, b[kk], acc[4]);
        acc[5] = mfma_f32(a1.y, b[kk], acc[5]);
        acc[6] = mfma_f32(a1.z, b[kk], acc[6]);
        acc[7] = mfma_f32(a1.w, b[kk], acc[7]);
        if (kk < 15) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);   // 2 LDS reads (k-step kk + 1)
        __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);                // 8 MFMAs (k-step kk)
        a0 = n0; a1 = n1;
    }
}

// act[ib][r] = LeakyReLU(acc[ib][r] + bias[channel]), acc = 0.  Registers 4 g .. 4 g + 3 of block ib = channels 32 ib + 8 g + 4 h + e
__device__ __forceinline__ void activate(f32x16 (&acc)[8], const float *bias, int h, float (&act)[8][16]) {
#pragma unroll
    for (int ib = 0; ib < 8; ib++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const float4 bv = *reinterpret_cast<const float4 *>(bias + 32 * ib + 8 * g + 4 * h);
            act[ib][4 * g + 0] = lrelu(acc[ib][4 * g + 0] + bv.x);
            act[ib][4 * g + 1] = lrelu(acc[ib][4 * g + 1] + bv.y);
            act[ib][4 * g + 2] = lrelu(acc[ib][4 * g + 2] + bv.z);
            act[ib][4 * g + 3] = lrelu(acc[ib][4 * g + 3] + bv.w);
        }
#pragma unroll
    for (int ib = 0; ib < 8; ib++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[ib][r] = 0.f;
}

// col[ob] += sum over 64 k-steps of W_chunk[ob][k-step] x act[4 C + k-step / 16][k-step % 16]: chunk C (input blocks 4 C .. 4 C + 3)
// of the 64-channel output layer fc_out_c
template <int C>
__device__ __forceinline__ void chunk_out2(const char *wbuf, int lane, const float (&act)[8][16], f32x16 (&col)[2]) {
    const float2v *w = reinterpret_cast<const float2v *>(wbuf) + lane;
#pragma unroll
    for (int kk = 0; kk < 64; kk++) {
        const float2v a = w[kk * 64];
        col[0] = mfma_f32(a[0], act[4 * C + (kk >> 4)][kk & 15], col[0]);
        col[1] = mfma_f32(a[1], act[4 * C + (kk >> 4)][kk & 15], col[1]);
    }
}

// ---- the layers of an MLP kernel -----------------------------------------------------------------------------------------------------
// The kernel's two weight buffers (two OBJECTS: see field_f32_kernel) and this lane's place in the workgroup.  Chunk n of the stream
// goes through buffer n & 1; a layer leaves the chunk behind its last one in flight or landed, as it found its own first.
struct WeightBuffers {
    const float *wpk;
    char *wb0, *wb1;
    int wave, lane;
    unsigned lane16;
};

// one 256 -> 256 layer: acc += W act, chunks c0 .. c0 + 7 of the stream (c0 even), chunk c0 + b = input block b
__device__ __forceinline__ void hidden_layer(const WeightBuffers &s, int c0, const float (&act)[8][16], f32x16 (&acc)[8]) {
#pragma unroll
    for (int b = 0; b < 8; b++) {
        chunk_fetch(s.wpk, (b & 1) ? s.wb0 : s.wb1, c0 + b + 1, s.wave, s.lane16);
        chunk_mul8((b & 1) ? s.wb1 : s.wb0, s.lane, act[b], acc);
        __syncthreads();
    }
}

// fc_out_c: col = W act + bias, chunks c0, c0 + 1 (c0 even); chunk `next` -- chunk 0 of the next pass -- is fetched behind them
__device__ __forceinline__ void out_layer(const WeightBuffers &s, int c0, int next, const float (&act)[8][16], const float *bias, int h,
                                          f32x16 (&col)[2]) {
    col[0] = zero16();
    col[1] = zero16();
    chunk_fetch(s.wpk, s.wb1, c0 + 1, s.wave, s.lane16);
    chunk_out2<0>(s.wb0, s.lane, act, col);
    __syncthreads();
    chunk_fetch(s.wpk, s.wb0, next, s.wave, s.lane16);
    chunk_out2<1>(s.wb1, s.lane, act, col);
    __syncthreads();
#pragma unroll
    for (int ib = 0; ib < 2; ib++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const float4 bv = *reinterpret_cast<const float4 *>(bias + 32 * ib + 8 * g + 4 * h);
            col[ib][4 * g + 0] += bv.x; col[ib][4 * g + 1] += bv.y; col[ib][4 * g + 2] += bv.z; col[ib][4 * g + 3] += bv.w;
        }
}

}  // namespace
