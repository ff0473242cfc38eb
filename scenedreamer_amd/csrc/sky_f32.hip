// The sky MLP in plain fp32 on the f32-input matrix instruction of gfx950 (v_mfma_f32_32x32x2_f32): SKYMLP.forward on PE(raydir)
// (imaginaire/generators/gancraft_base.py:150-169; positional encoding .../voxlib/positional_encoding_kernel.cu:40-75) for every
// ray of the frame + the frame mean (scenedreamer.py:592-598), like sky.hip -- but every product is an f32 x f32 fmaf (the MFMA
// result is bit for bit a k-ordered fmaf chain): the weights have fp32's RANGE (no 2^8-scaled f16 stream, no TrunkRangeError),
// nothing is calibrated, and no bit depends on a library's choice of solver or summation order.  It is the sky of the exact
// rung (field_f32.hip, cnn_f32.hip), not the default: on weights sky_kernel accepts it is no closer to fp64 than sky_kernel is.
//
//   sky_f32_kernel<PRE>    32 rays per wave as the 32 columns of the B operand (lanes, streams and chunk pipeline: mlp_f32.h), 4 waves = a 128-ray
//                          group per workgroup, groups grid-strided.  fc1 + style bias -> fc2 .. fc5 -> fc_out_c; activations stay
//                          in registers.  PRE = false: ray directions [n,3], encoded here by posenc_enc.h (the op's own function);
//                          PRE = true: SKYMLP.forward's argument [n,33].  Both give the same bits on the op's encoding.
//   sky_pack_f32_kernel    every weight once, in the order the kernel consumes them.
//
// Weights: 36 chunks per group (2 fc1, 8 per hidden layer, 2 fc_out_c).  fc1 has K = 33: it is padded to K = 64, TWO full chunks,
// with zero weights and zero inputs (fmaf(0, 0, acc) is acc: exact).  Cost: 256 MFMAs for fc1 where 17 k-steps x 8 blocks = 136 would do, 120 of 4608 = 2.6 % of the matrix issue
// (arithmetic).  One chunk plus a one-k-step tail would save them, for a 34 KiB chunk that does not fit the 32 KiB buffers or a
// second kind of fetch; the uniform chunk loop was kept.
// Frame mean: the 32 rays of a tile are added in f32 as a depth-5 tree (the DPP / __shfl_xor sequence of sky_kernel); every
// accumulation after that is f64 -- the per-lane running sums over a workgroup's groups, one partial row per wave, and the
// row-ordered total of the last workgroup to arrive (sky_kernel's arrival protocol: no float atomics), which writes
// sky_avg = (float)(sum / n) and resets the counter.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), one wave per SIMD:
//   sky_f32_kernel<false>  176 VGPRs + 128 AGPRs, 0 B scratch, no spill, 72 968 B LDS
//   sky_f32_kernel<true>   174 VGPRs + 128 AGPRs, 0 B scratch, no spill, 72 968 B LDS
#include "mlp_f32.h"
#include "posenc_enc.h"
#include "sdn_common.h"

namespace {

constexpr int SKY_F32_CHUNKS = 2 + 4 * 8 + 2;   // fc1 (K padded to 64) | fc2 .. fc5 | fc_out_c; even, so a chunk's buffer is its index & 1
constexpr size_t SKY_F32_FLOATS = (size_t)SKY_F32_CHUNKS * CHUNK_FLOATS;
static_assert(SKY_F32_FLOATS == (size_t)HID * SKY_K0 + 4 * HID * HID + OUTC * HID, "the stream holds every weight once (fc1 padded to K = 64)");
constexpr int SKY_DEG = 5;                      // positional_encoding(raydirs, 5, incl_orig): 2 * 5 * 3 + 3 = SKY_IN
static_assert(SKY_IN == 6 * SKY_DEG + 3 && SKY_K0 == 64, "fc1's input");

// the constant block of sdn_sky_consts_floats() (sky.hip)
constexpr int SC_BIAS1 = 0;                     // [256] fc1.bias + fc_z_a(z)
constexpr int SC_BIASH = 256;                   // [4][256] fc2..fc5 bias
constexpr int SC_BC = SC_BIASH + 4 * 256;       // [64]
constexpr int SC_TOTAL = SC_BC + 64;

struct SkyF32Params {
    const float *in;        // [R,3] ray directions, or (PRE) [R,33] positional-encoded rows
    const float *wpk;       // packed f32 weights (sky_pack_f32_kernel)
    const float *consts;    // SC_TOTAL floats
    float *sky_c;           // [R,64]
    double *sky_partial;    // [4 * gridDim.x][64]: every wave's sum of sky_c over its rays
    float *sky_avg;         // optional [64]: the frame mean, finished by the last workgroup to arrive
    unsigned int *counter;  // with sky_avg: arrival counter, zero before the first launch (the kernel leaves it at zero)
    int32_t R, n_tiles;
};

template <bool PRE>
__global__ __launch_bounds__(256, 1) void sky_f32_kernel(const SkyF32Params p) {
    // two OBJECTS, as in field_f32_kernel: the LDS-DMA into one cannot alias the fragment reads from the other
    __shared__ __attribute__((aligned(1024))) char wb0[CHUNK_BYTES];
    __shared__ __attribute__((aligned(1024))) char wb1[CHUNK_BYTES];
    __shared__ __attribute__((aligned(16))) float cst[SC_TOTAL];
    __shared__ double red[256];
    __shared__ int ticket;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31, q = j & 3;
    const unsigned lane16 = lane * 16;
    const WeightBuffers ws{p.wpk, wb0, wb1, wave, lane, lane16};

    chunk_fetch(p.wpk, wb0, 0, wave, lane16);
    for (int i = threadIdx.x; i < SC_TOTAL; i += 256) cst[i] = p.consts[i];
    __syncthreads();   // chunk 0 and the constants are in place.  From here on: at a group's start chunk 0 sits in buffer 0

    double fsum[2][4] = {{0., 0., 0., 0.}, {0., 0., 0., 0.}};   // lane (q, h) owns features 32 ib + 8 q + 4 h + e
    const int n_groups = (p.n_tiles + 3) >> 2;
    for (int grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const int tile = grp * 4 + wave;
        const int ray = tile * 32 + j;
        const bool ray_ok = tile < p.n_tiles && ray < p.R;
        const int rr = ray_ok ? ray : p.R - 1;     // (rays past the end evaluate the last ray, store nothing)

        // ---- fc1's input: b[t] = encoded element 2 t + h, t = 0 .. 16; zero beyond -----------------------------------------------
        float b0[16], b32;
        if constexpr (PRE) {
            const float *src = p.in + (size_t)rr * SKY_IN + h;
#pragma unroll
            for (int t = 0; t < 16; t++) b0[t] = src[2 * t];
            const float last = p.in[(size_t)rr * SKY_IN + 32];     // (read by both halves: no address past the row)
            b32 = h ? 0.f : last;
        } else {
            const float d[3] = {p.in[(size_t)rr * 3], p.in[(size_t)rr * 3 + 1], p.in[(size_t)rr * 3 + 2]};
            float pe[SKY_IN];     // [sin_0(3) cos_0(3) ... sin_4(3) cos_4(3) d(3)]
#pragma unroll
            for (int i = 0; i < SKY_DEG; i++)
#pragma unroll
                for (int c = 0; c < 3; c++) posenc_sincos(d[c], i, pe[6 * i + c], pe[6 * i + 3 + c]);
            pe[30] = d[0]; pe[31] = d[1]; pe[32] = d[2];
#pragma unroll
            for (int t = 0; t < 16; t++) {
                // (opaque copies: of plain array reads hipcc makes pe[2 t + h], a dynamic index, and moves pe to scratch memory)
                float ev = pe[2 * t], od = pe[2 * t + 1];
                asm volatile("" : "+v"(ev), "+v"(od));
                b0[t] = h ? od : ev;
            }
            b32 = h ? 0.f : pe[32];
        }

        f32x16 acc[8];
#pragma unroll
        for (int ib = 0; ib < 8; ib++) acc[ib] = zero16();
        float act[8][16];
        // ---- fc1: chunks 0, 1 ------------------------------------------------------------------------------------------------------
        chunk_fetch(p.wpk, wb1, 1, wave, lane16);
        chunk_mul8(wb0, lane, b0, acc);
        __syncthreads();
        {
            float b1[16];
            b1[0] = b32;
#pragma unroll
            for (int t = 1; t < 16; t++) b1[t] = 0.f;
            chunk_fetch(p.wpk, wb0, 2, wave, lane16);
            chunk_mul8(wb1, lane, b1, acc);
            __syncthreads();
        }
        activate(acc, cst + SC_BIAS1, h, act);          // fc1(x) + fc_z_a(z), gancraft_base.py:158-162
        // ---- fc2 .. fc5: chunks 2 + 8 l + b, b = input block -----------------------------------------------------------------------
#pragma unroll 1
        for (int l = 0; l < 4; l++) {
            hidden_layer(ws, 2 + 8 * l, act, acc);
            activate(acc, cst + SC_BIASH + l * HID, h, act);
        }
        // ---- fc_out_c: chunks 34, 35, and chunk 0 of the next group behind them; sky_c[ray] ---------------------------------------------
        f32x16 col[2];
        out_layer(ws, SKY_F32_CHUNKS - 2, 0, act, cst + SC_BC, h, col);
        if (ray_ok) store_colour_row(p.sky_c + (size_t)ray * OUTC, col, h);
        // ---- the tile's 32 rays added in f32, a depth-5 tree (sky_kernel's sequence: quad, half-row mirror, row mirror within a
        //      row of 16 lanes, one exchange for the other row); from here on f64 -------------------------------------------------------
#pragma unroll
        for (int ib = 0; ib < 2; ib++)
#pragma unroll
            for (int rg = 0; rg < 16; rg++) {
                float v = ray_ok ? col[ib][rg] : 0.f;
                v += quad_dpp<QUAD_XOR1>(v);
                v += quad_dpp<QUAD_XOR2>(v);
                v += quad_dpp<DPP_ROW_HALF_MIRROR>(v);
                v += quad_dpp<DPP_ROW_MIRROR>(v);
                v += __shfl_xor(v, 16);
                if ((rg >> 2) == q) fsum[ib][rg & 3] += (double)v;
            }
    }
    __syncthreads();   // (a group's last fetch -- chunk 0 for a group that never came -- lands before the LDS is released)
    // lanes with j < 4 (q = j) of each half hold the sums of features 32 ib + 8 q + 4 h + e
    if (j < 4) {
#pragma unroll
        for (int ib = 0; ib < 2; ib++)
#pragma unroll
            for (int e = 0; e < 4; e++)
                p.sky_partial[(size_t)(blockIdx.x * 4 + wave) * OUTC + 32 * ib + 8 * q + 4 * h + e] = fsum[ib][e];
    }
    // ---- frame mean (scenedreamer.py:592-598): the last workgroup to arrive adds the partial rows of ALL workgroups in row
    //      order, in f64 (fixed order: reproducible bit for bit) ---------------------------------------------------------------------
    if (p.sky_avg == nullptr) return;
    __threadfence();                                               // this workgroup's rows are visible device-wide ...
    __syncthreads();                                               // (... every wave's)
    if (threadIdx.x == 0) ticket = (int)atomicAdd(p.counter, 1u);  // ... before its arrival is counted
    __syncthreads();
    if (ticket != (int)gridDim.x - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const int rows = 4 * (int)gridDim.x, f = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int r0 = part * (rows / 4), r1 = r0 + rows / 4;          // four consecutive quarters of the rows
    double acc_d = 0.0;
    for (int rw = r0; rw < r1; rw++) acc_d += __builtin_nontemporal_load(p.sky_partial + (size_t)rw * OUTC + f);
    red[threadIdx.x] = acc_d;
    __syncthreads();
    if (threadIdx.x < OUTC) {
        const double tot = ((red[f] + red[64 + f]) + red[128 + f]) + red[192 + f];
        p.sky_avg[f] = (float)(tot / (double)p.R);
    }
    if (threadIdx.x == 0) *p.counter = 0u;                         // ready for the next launch
}

// ---- the packed stream --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sky_pack_f32_kernel(const MlpPackF32<4> p) {   // w1 [256,33]; wh: fc2 .. fc5
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;   // one thread per float of the stream
    if (g >= SKY_F32_FLOATS) return;
    p.out[g] = mlp_stream_weight<2>(p, g, [&](int cp, ChunkPos s) {
        const int k = 2 * (16 * cp + s.kk) + s.h;
        return k < SKY_IN ? p.w1[(size_t)s.row * SKY_IN + k] : 0.f;
    });
}

int sky_f32_workgroups(int32_t n_rays, int32_t n_workgroups) {
    const int wg = n_workgroups > 0 ? n_workgroups : 256;
    const int groups = sdn::div_up(sdn::div_up(n_rays, 32), 4);
    return wg > groups ? groups : wg;
}

}  // namespace

extern "C" {

size_t sdn_sky_f32_packed_weight_bytes(void) { return SKY_F32_FLOATS * sizeof(float); }

int sdn_sky_pack_weights_f32(const float *w1, const float *const *wh4_host, const float *wc, void *packed, sdn_stream_t stream) {
    return pack_mlp_weights_f32<4>("sdn_sky_pack_weights_f32", sky_pack_f32_kernel, SKY_F32_FLOATS, w1, wh4_host, wc, packed, stream);
}

int32_t sdn_sky_f32_partial_rows(int32_t n_rays, int32_t n_workgroups) { return n_rays > 0 ? 4 * sky_f32_workgroups(n_rays, n_workgroups) : 0; }

int sdn_sky_mlp_f32(const float *raydirs, const void *packed, const float *consts, float *sky_c, double *sky_partial, int32_t n_rays,
                    int32_t n_workgroups, float *sky_avg, uint32_t *counter, int32_t encoded, sdn_stream_t stream) {
    SDN_REQUIRE(raydirs && packed && consts && sky_c && sky_partial && n_rays > 0, "sdn_sky_mlp_f32: bad argument");
    SDN_REQUIRE((sky_avg == nullptr) == (counter == nullptr), "sdn_sky_mlp_f32: sky_avg and counter go together");
    SDN_REQUIRE(encoded == 0 || encoded == 1, "sdn_sky_mlp_f32: encoded must be 0 (ray directions) or 1 (positional-encoded rows)");
    if (sdn_sky_consts_floats() != (size_t)SC_TOTAL) return sdn::fail(SDN_ERR_INVALID, "sdn_sky_mlp_f32: constant block layout differs from sdn_sky_mlp's");
    SkyF32Params p;
    p.in = raydirs; p.wpk = (const float *)packed; p.consts = consts; p.sky_c = sky_c; p.sky_partial = sky_partial;
    p.sky_avg = sky_avg; p.counter = counter;
    p.R = n_rays;
    p.n_tiles = sdn::div_up(n_rays, 32);
    const int wg = sky_f32_workgroups(n_rays, n_workgroups);
    if (encoded) hipLaunchKernelGGL((sky_f32_kernel<true>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((sky_f32_kernel<false>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p);
    return sdn::check_launch("sdn_sky_mlp_f32");
}

}  // extern "C"
