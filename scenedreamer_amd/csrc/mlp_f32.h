// The fp32 layer code of the register-resident MLPs on the f32-input matrix instruction of gfx950 (v_mfma_f32_32x32x2_f32),
// shared by the field (field_f32.hip) and the sky MLP (sky_f32.hip): every product is an f32 x f32 fmaf, the MFMA result is bit
// for bit a k-ordered fmaf chain.  All of it is per translation unit (anonymous namespace, force-inlined), like mlp_layers.h.
//
// Layout.  A layer is evaluated transposed, W as the A operand (32 output channels per block), 32 rows (samples, rays) as the
// columns.  Lane l = (h = l >> 5, j = l & 31) holds A[i = j][k = h] and B[k = h][col j], one f32 each; accumulator register r of
// lane (h, j) holds channel 8 (r / 4) + 4 h + r % 4 of column j.  The packed weights order the k-steps of every hidden layer so
// that k-step r of input block b pairs channels 32 b + 8 (r / 4) + r % 4 (h = 0) and ... + 4 (h = 1) (kmap_f32): accumulator
// register r of block b, after bias + LeakyReLU, IS the B operand of that k-step.  Activations never leave the registers and
// never cross lanes.
// Weights come in chunks of 32 KiB: 16 k-steps of an 8-block layer (chunk_mul8), or 64 k-steps of the 2-block output layer
// (chunk_out2).  The four waves of a workgroup share one copy: chunk n + 1 is copied L2 -> LDS (global_load_lds, 16 B per lane,
// lane-linear image) into the second buffer while chunk n is multiplied; one __syncthreads() per chunk ends both.
#pragma once
#include "mlp_layers.h"

namespace {

constexpr int CHUNK_BYTES = 32768;
constexpr int CHUNK_FLOATS = CHUNK_BYTES / 4;

__device__ __forceinline__ float lrelu(float x) { return x > 0.f ? x : 0.2f * x; }   // F.leaky_relu(x, 0.2)

__device__ __forceinline__ f32x16 mfma_f32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// channel that accumulator register r of lane half h holds inside its 32-channel block = k of k-step r of that input block
__host__ __device__ inline int kmap_f32(int r, int h) { return 8 * (r >> 2) + 4 * h + (r & 3); }

template <int K>
__device__ __forceinline__ void chunk_piece(const char *lane_src, char *dst) {
    // the immediate offset (a 13-bit signed field: below 4096) is added to the global AND to the LDS address
    __builtin_amdgcn_global_load_lds((glb_char *)(lane_src + (K / 4) * 4096), (lds_char *)(dst + (K / 4) * 4096), 16, (K % 4) * 1024, 0);
}

// this wave's quarter of chunk `cp` of the stream -> weight buffer cp & 1: 8 pieces of 1 KiB (64 lanes x 16 B).
// The source address is a uniform base + this lane's 32-bit byte offset (the saddr form of the load): as 64-bit per-lane
// pointers hipcc hoists the 8 addresses of every call out of the pass loop and keeps them in scratch memory.
__device__ __forceinline__ void chunk_fetch(const float *wpk, char *wbuf, int cp, int wave, unsigned lane16) {
    const char *src = reinterpret_cast<const char *>(wpk) + (size_t)cp * CHUNK_BYTES + wave * 8192;    // uniform
    char *dst = wbuf + wave * 8192;      // wave-uniform; the DMA adds lane * 16
    asm volatile("" : "+v"(lane16));
    chunk_piece<0>(src + lane16, dst); chunk_piece<1>(src + lane16, dst); chunk_piece<2>(src + lane16, dst); chunk_piece<3>(src + lane16, dst);
    chunk_piece<4>(src + lane16, dst); chunk_piece<5>(src + lane16, dst); chunk_piece<6>(src + lane16, dst); chunk_piece<7>(src + lane16, dst);
}

// acc[ib] (+)= sum over 16 k-steps of W_chunk[ib][k-step] x b[k-step]: one chunk of an 8-block layer.  A k-step's 2 KiB in the
// chunk: [output blocks 0-3 | 4-7][lane][4 blocks], so a lane reads two float4 (conflict-free, lane-linear)
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
// of the 64-channel output layer fc_out_c; a k-step is [lane][2 output blocks]
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

}  // namespace
