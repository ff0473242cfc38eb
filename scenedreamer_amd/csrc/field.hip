// Fused field renderer for gfx950: sample placement -> hash-grid lookup -> style-modulated MLP on
// MFMA -> volume rendering + sky compositing.  Fast path for the reference's
// Generator._forward_perpix / _forward_perpix_sub (imaginaire/generators/scenedreamer.py:285-430)
// with mc_utils.sample_depth_batched (:82-151), GridEncoder.forward (gridencoder/grid.py:140-156),
// LightningMLP.forward (imaginaire/model_utils/layers.py:92-126) and volum_rendering_relu
// (mc_utils.py:154-161).
//
// Kernels
//   collapse_kernel   once per scene.  The two trailing hash-grid coordinates (global_enc) are
//                     constant per scene, and every level is hashed into a power-of-two table, so
//                     (h ^ K) & m == (h & m) ^ (K & m) and the 32-corner 5-D blend factorises exactly
//                     into an 8-corner 3-D blend of a per-scene table
//                        T'[l][i] = sum_{c3,c4} w3 w4 T[l][i ^ K(c3,c4)]
//                     (SURVEY.md appendix A).  4x fewer gathers per sample; only the fp32 summation
//                     order differs from the reference.
//   encode_kernel     per frame, one wave per 8 rays, 4 samples of every ray per step (32 MFMA columns):
//                     places the samples (bit-identical decisions to the reference), blends the 16
//                     levels from the collapsed table and writes the features as the MLP's B fragments,
//                     already split into f16 hi / lo.  Reads the frame-wide ray arrays through a ray window.
//                     Pure gather: bound by L2 / Infinity-Cache / HBM bandwidth.
//   mlp_kernel        per frame, persistent, one wave per SIMD (4 per CU), 32 samples per wave step.
//                     The MLP is evaluated TRANSPOSED: D^T[feature][sample] = W[feature][k] * X[k][sample],
//                     weights are the MFMA A operand, samples the B operand.  A wave keeps all 256
//                     activations of its 32 samples in registers; the C/D register layout of one layer is
//                     consumed directly as the B layout of the next (the k-permutation this implies is
//                     baked into the packed weights), so activations never touch LDS or HBM.
//                     Precision: the north star demands 1e-3 abs on radiance and the density head
//                     amplifies hidden-activation error by ~1e2, which plain f16/bf16 MFMA misses by 10x
//                     (measured).  Every product is therefore evaluated as a 3-term split
//                     (Whi*Xhi + Wlo*Xhi + Whi*Xlo, f32 accumulate): ~2^-21 relative error at 3 f16 MFMAs
//                     per tile, 5.3x the rate of the f32 MFMA.  In the colour layers fc_5 / fc_6, whose error
//                     nothing amplifies, the two correction terms run as block-scaled fp6 products
//                     (v_mfma_scale_f32_32x32x64_f8f6f4: K = 64 at the issue cost of a K = 16 f16 MFMA).
//                     Volume rendering, the density head, label bias, clamp and sky blend run in the
//                     epilogues on the VALU.  The persistent workgroups draw their 32-ray groups from a
//                     ticket counter; groups whose rays all miss are skipped.
//   field_kernel      = mlp_kernel<.., FUSED>: the north star's "hash-grid lookup plus the MLP fused into ONE kernel".  Every
//                     pass starts with the encode stage of its own 32 samples (sample placement + collapsed-table gathers,
//                     the very device functions encode_kernel is made of) executed by the MLP wave into its B-fragment
//                     registers -- a lane's 8 levels x 8 channels ARE its 8 B fragments, so nothing is exchanged -- while the
//                     accumulator / fragment-ring registers are dead.  No feature buffer, no 10.8 GB HBM round trip.
//   sample_depth_kernel   mc_utils.sample_depth_batched as an op of its own.
//   mfma_probe_kernel     checks the MFMA operand layouts the layer machinery relies on.
// The encode stage's device functions (ray window, sample placement, collapsed-table gathers) are in field_enc.h, what a field
// kernel does around its MLP (LDS prologue, volume rendering, sky compositing, launch helpers) in field_composite.h: both shared
// with the fp32 field kernel (field_f32.hip).  The layer machinery (weight ring, activation stages, layers) is in mlp_layers.h, the weight packers (pack_kernel,
// pack_mx_kernel) in mlp_pack.hip; the sky MLP (sky.hip) and the render CNN's 1x1 ends (cnn_ends.hip) run on them too.
#include <hip/hip_fp16.h>

#include <cstdlib>
#include <utility>

#include "field_composite.h"
#include "mlp_layers.h"
#include "sdn_common.h"

namespace {

typedef int i32x4v __attribute__((ext_vector_type(4)));

struct MlpParams {
    const float *feat;
    const float *dist;
    const uint8_t *label;
    const uint8_t *rayflag;
    const half8 *wpk;          // packed weights
    const float *consts;       // fp32 constant block
    const float *sky_c;        // [R, 64] sky_net output per ray
    float *net_out;            // [R, 64]
    int32_t R, ns, nch, n_tiles;
    float term_depth;          // early ray termination: optical depth -ln(eps) beyond which a ray is opaque; <= 0: off
    uint8_t *passes;           // optional [ceil(n_tiles / 4)]: passes every 32-ray group went through (tests / bench)
    RayWindow win;             // sky_c is indexed with the SOURCE ray (it covers the whole padded frame)
    const float *sky_avg;      // optional dev [64]: frame mean of sky_c (else the value inside `consts`)
    int32_t *ticket;           // optional dev int32[2], zero before the first launch (the kernel leaves it zero): the
                               // persistent workgroups draw their 32-ray groups from it instead of taking every
                               // gridDim.x-th one (a static share that is mostly sky leaves its workgroup idle at the end)
    EncParams enc;             // FUSED (field_kernel): the encode stage's inputs; feat / dist / label / rayflag are unused then
    const float *cam_ori_dev;  // FUSED, optional dev f32 [3]: the camera origin read from device memory (overrides enc.ori): callers that hold
                               // it as a device tensor (Generator._forward_perpix's cam_ori_t) need no device -> host copy per call
    // MODE_FUSED_AUX: the other return values of Generator._forward_perpix (scenedreamer.py:429-430), each optional
    float *w_out;              // [R][ns]     weights: volume-rendering weight of every sample, * !sky_only (:373-376)
    float *depth_out;          // [R][ns]     rand_depth after the NaN / inf -> 0 replacement (:350-352)
    float *sig_out;            // [R][ns]     net_out_s: fc_sigma's output per sample (layers.py:114)
    float *col_out;            // [R][ns][64] net_out_c: fc_out_c's output per sample (layers.py:124)
    float *skyb_out;           // [R][64]     skynet_out_c after the keep_sky_out blend with sky_avg (:401)
    uint8_t *nosky_out;        // [R]         nosky_mask (:382-383)
    float *sigma_out;          // MODE_RAW: [R] density fc_sigma(f) of every row (LightningMLP.forward's first output)
    uint8_t *colour_passes;    // optional [ceil(n_tiles / 4)]: passes of every 32-ray group that ran the colour branch (tests / bench)
    int32_t no_colour_skip;    // field_kernel: 1 = evaluate fc_5 / fc_6 / fc_out_c in every pass (A/B switch; the results are identical)
};

// mlp_kernel's input / output modes
constexpr int MODE_BUFFER = 0;      // features from encode_kernel's buffer
constexpr int MODE_FUSED = 1;       // field_kernel: every pass encodes its own samples
constexpr int MODE_FUSED_AUX = 2;   // field_kernel that also writes the per-sample weights and depths (Generator._forward_perpix's
                                    // `weights` / `rand_depth` outputs, used by inference_givenstyle_depth, scenedreamer.py:812-817)
constexpr int MODE_RAW = 3;         // LightningMLP.forward as an op (imaginaire/model_utils/layers.py:92-126): rows of 128 f32 features
                                    // + a label per row in, (sigma, colour features) per row out; no sample placement, no compositing.
                                    // Row (tile, ch, j) = tile * 256 + ch * 32 + j: `R` counts rows, nch = 8, a tile = 256 rows.

// =====================================================================================================
// collapse
// =====================================================================================================
struct CollapseParams {
    const float *emb;   // original table, level l at emb + off[l] * 8
    float *table3;
    uint32_t T;
    uint32_t off[NLEV];
    uint32_t K[NLEV][4];   // hash contribution of corner (c3, c4), index c3 + 2*c4, already & (T-1)
    float w[NLEV][4];      // w3 * w4 with the reference's multiply order
};

__global__ __launch_bounds__(256) void collapse_kernel(const CollapseParams p) {
    const uint32_t level = blockIdx.y;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.T) return;
    const float *src = p.emb + (size_t)p.off[level] * 8;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; c++) {  // c3 fastest, like the corner index of the reference loop
        const float4 a = *reinterpret_cast<const float4 *>(src + (size_t)(i ^ p.K[level][c]) * 8);
        const float4 b = *reinterpret_cast<const float4 *>(src + (size_t)(i ^ p.K[level][c]) * 8 + 4);
        const float w = p.w[level][c];
        acc[0] += w * a.x; acc[1] += w * a.y; acc[2] += w * a.z; acc[3] += w * a.w;
        acc[4] += w * b.x; acc[5] += w * b.y; acc[6] += w * b.z; acc[7] += w * b.w;
    }
    float *dst = p.table3 + ((size_t)level * p.T + i) * 8;
    *reinterpret_cast<float4 *>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *reinterpret_cast<float4 *>(dst + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
}

// =====================================================================================================
// encode: sample placement + collapsed hash-grid lookup (the per-sample device functions: field_enc.h)
// =====================================================================================================
#ifndef SDN_ENC_OCC
#define SDN_ENC_OCC 3   // 3 waves per SIMD = up to 168 VGPRs: no spills (with 1, hipcc aims at 4 waves and spills 100 B; 4 and 5 measured slower)
#endif
__global__ __launch_bounds__(256, SDN_ENC_OCC) void encode_kernel(const EncParams p) {
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= p.n_tiles) return;
    const int h = lane >> 5, j = lane & 31;
    const int ray = tile * RAYS_PER_TILE + (j >> 2);
    const bool ray_ok = ray < p.R && p.win.valid(ray);
    const int rl = ray_ok ? ray : p.R - 1;      // local ray (index into u / rayflag)
    const int rr = p.win.src(rl);               // the same ray in the source arrays

    RayBoxes rb;
    float d[3];
    enc_load_ray(p, rr, rb, d);
    bool gnd = false;
    // A ray that hits nothing gets weight 0 for all its samples (scenedreamer.py:376: weights * (1 - sky_only)), so
    // its features are never used: no gathers for its lanes, and no feature traffic at all for a tile of 8 such rays
    // (the MLP kernel reads whatever is there and discards the result by selection, not multiplication).
    const bool use_feat = ray_ok && rb.id[0] != 0;
    const bool tile_dead = !__any(use_feat);

    for (int ch = 0; ch < p.nch; ch++) {
        const EncSample e = enc_place(p, rb, d, rl, ch * SAMP_PER_STEP + (j & 3), ray_ok);
        if (e.gnd) gnd = true;
        const size_t tc = (size_t)tile * p.nch + ch;
        if (h == 0) {
            p.dist[tc * 32 + j] = e.dist;
            p.label[tc * 32 + j] = (uint8_t)e.label;
        }
        if (tile_dead) continue;
        float *fout = p.feat + (tc * 8 * 64 + lane) * 8;
#pragma unroll 2
        for (int s = 0; s < 8; s++) {
            float res[8];
            enc_level(p, e, 2 * s + h, use_feat, res);
            float *o = fout + (size_t)s * 64 * 8;
            // The features leave as the MLP's operands: the 8 values of this lane's B fragment split into f16 hi (first
            // 16 bytes) and f16 lo (second 16 bytes) -- the same 32 bytes per lane and k-step as 8 floats, and exactly the
            // split mlp_kernel used to do at every pass start (128 VALU instructions of a wave that has no issue slots to
            // spare; this kernel waits for gathers anyway).
            // Streaming stores: the 4.9 GB of features are written once and read once by the MLP kernel; they should not
            // displace the collapsed table (the gathers' working set) from L2 / Infinity Cache
            half8 hi8, lo8;
            split8(res, hi8, lo8);
            typedef unsigned int u4v __attribute__((ext_vector_type(4)));
            __builtin_nontemporal_store(__builtin_bit_cast(u4v, hi8), reinterpret_cast<u4v *>(o));
#ifndef SDN_ENC_HI_ONLY   // (timing ablation: upper bound of what fewer feature bytes can buy)
            __builtin_nontemporal_store(__builtin_bit_cast(u4v, lo8), reinterpret_cast<u4v *>(o + 4));
#endif
        }
    }
    // per-ray flags: any over the ray's 4 lanes
    gnd = quad_dpp<QUAD_XOR1>((int)gnd) | (int)gnd;
    gnd = quad_dpp<QUAD_XOR2>((int)gnd) | (int)gnd;
    if (h == 0 && (j & 3) == 0 && ray_ok) {
        const bool sky_only = rb.id[0] == 0;             // scenedreamer.py:337
        int last = rb.id[0];
#pragma unroll
        for (int k = 1; k < MAXM; k++)
            if (k == p.M - 1) last = rb.id[k];
        const bool nosky = (last != 0) || gnd;           // :335, :382
        p.rayflag[ray] = (uint8_t)((sky_only ? 1 : 0) | (nosky ? 2 : 0));
    }
}

// =====================================================================================================
// mc_utils.sample_depth_batched as an op of its own (the un-fused path and training): one thread per ray
// =====================================================================================================
struct SampleParams {
    const float *depth2;   // [2, R, M]
    const float *lin;      // [n_points]
    const float *u;        // [R, n_points] or nullptr
    float *rand_depth;     // [R, n_points - 1]
    float *new_dists;      // [R, n_points - 1]
    int64_t *idx;          // [R, n_points - 1]
    int32_t R, M, n_points;
    int32_t ieee_div;
    float sample_depth;
};

__global__ __launch_bounds__(256) void sample_depth_kernel(const SampleParams p) {
    const int ray = blockIdx.x * 256 + threadIdx.x;
    if (ray >= p.R) return;
    RayBoxes rb;
#pragma unroll
    for (int k = 0; k < MAXM; k++) {
        if (k < p.M) {
            rb.t[k] = p.depth2[(size_t)ray * p.M + k];
            rb.t2[k] = p.depth2[((size_t)p.R + ray) * p.M + k];
        } else {
            rb.t[k] = rb.t2[k] = __builtin_nanf("");
        }
        rb.id[k] = 0;
    }
    const float *u = p.u ? p.u + (size_t)ray * p.n_points : nullptr;
    const int ns = p.n_points - 1;
    for (int i = 0; i < ns; i++) {
        Placed pl = place_sample(rb, p.M, p.lin, u, p.ieee_div ? -p.n_points : p.n_points, i, p.sample_depth);
        // the op returns the RAW values: NaN depths of rays that hit nothing are zeroed by the caller (scenedreamer.py:350-352)
        // and the box index is the count itself, mc_utils.py:139 (place_sample clamps it for the label lookup)
        p.new_dists[(size_t)ray * ns + i] = pl.dist;
        p.rand_depth[(size_t)ray * ns + i] = pl.raw_depth;
        p.idx[(size_t)ray * ns + i] = pl.raw_idx;
    }
}

// =====================================================================================================
// MLP + compositing (the structure of a pass and the layers: mlp_layers.h)
// =====================================================================================================
// ---- the input stage of a pass, a function per mode (MODE_RAW's few lines: in the kernel): the wave's 32 samples as B fragments bh / bl (fragment s of lane half h =
// ---- features 16 s + 8 h .. + 7, split into f16 hi / lo), and this lane's sample's label and distance ---------------------------------
// MODE_FUSED / _AUX: the encode stage of THIS pass (sample `sidx` of local ray rl = source ray rr), by this wave, into its own
// B-fragment registers (the accumulators, the fragment ring and the fp6 state are dead here, so the gathers of several levels
// can be in flight).  The loads are ordinary ones: hipcc's own vmcnt waits also retire the ring DMAs issued before them
// (vector memory completes in order) -- a stricter wait than the ring's counted ones, never a wrong one.
// gnd |= the sample lies at world x <= 1; depth = its rand_depth (the AUX kernel returns it)
__device__ __forceinline__ void input_encode(const EncParams &enc, int rr, int rl, int sidx, bool ray_ok, bool use_feat, int h, half8 (&bh)[16],
                                             half8 (&bl)[16], int &lab, float &dist, bool &gnd, float &depth) {
    RayBoxes rb;
    float dd[3];
    enc_load_ray(enc, rr, rb, dd);
    const EncSample es = enc_place(enc, rb, dd, rl, sidx, ray_ok);
    gnd = gnd || es.gnd;
    lab = es.label;
    dist = es.dist;
    depth = es.depth;
    // 4 levels' gathers (64 x 16 B per lane) in flight at a time: two round trips per pass instead of eight
#pragma unroll
    for (int b = 0; b < 2; b++) {
        float res[4][8];
        enc_levels<4>(enc, es, 4 * b, h, use_feat, res);
#pragma unroll
        for (int t = 0; t < 4; t++) split8(res[t], bh[4 * b + t], bl[4 * b + t]);
    }
}

// MODE_BUFFER: step tc of encode_kernel's feature buffer.  prefetched: input_prefetch(tc) was this wave's last prefetch -- the
// step sits in a[190:255]; else (first pass of the kernel / after a skipped group) it is loaded here
template <int DBG>
__device__ __forceinline__ void input_buffer(const MlpParams &p, size_t tc, bool prefetched, bool tile_ok, int lane, int j, half8 (&bh)[16],
                                             half8 (&bl)[16], int &lab, float &dist) {
    float raw[8][8];
    if (prefetched) {
        if constexpr (DBG & 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
#define SDN_PF_READ8(S, A0, A1, A2, A3, A4, A5, A6, A7) \
    asm volatile("v_accvgpr_read_b32 %0, a" #A0 "\n\tv_accvgpr_read_b32 %1, a" #A1 "\n\tv_accvgpr_read_b32 %2, a" #A2 \
                 "\n\tv_accvgpr_read_b32 %3, a" #A3 "\n\tv_accvgpr_read_b32 %4, a" #A4 "\n\tv_accvgpr_read_b32 %5, a" #A5 \
                 "\n\tv_accvgpr_read_b32 %6, a" #A6 "\n\tv_accvgpr_read_b32 %7, a" #A7 \
                 : "=v"(raw[S][0]), "=v"(raw[S][1]), "=v"(raw[S][2]), "=v"(raw[S][3]), "=v"(raw[S][4]), "=v"(raw[S][5]), \
                   "=v"(raw[S][6]), "=v"(raw[S][7]))
        SDN_PF_READ8(0, 190, 191, 192, 193, 194, 195, 196, 197);
        SDN_PF_READ8(1, 198, 199, 200, 201, 202, 203, 204, 205);
        SDN_PF_READ8(2, 206, 207, 208, 209, 210, 211, 212, 213);
        SDN_PF_READ8(3, 214, 215, 216, 217, 218, 219, 220, 221);
        SDN_PF_READ8(4, 222, 223, 224, 225, 226, 227, 228, 229);
        SDN_PF_READ8(5, 230, 231, 232, 233, 234, 235, 236, 237);
        SDN_PF_READ8(6, 238, 239, 240, 241, 242, 243, 244, 245);
        SDN_PF_READ8(7, 246, 247, 248, 249, 250, 251, 252, 253);
#undef SDN_PF_READ8
        asm volatile("v_accvgpr_read_b32 %0, a254\n\tv_accvgpr_read_b32 %1, a255" : "=v"(lab), "=v"(dist));
        if (!tile_ok) dist = 0.f;
    } else {
        // Inline asm as well, so that hipcc's wait insertion sees no vector-memory loads at all in the pass loop (with ordinary
        // loads on this path it puts vmcnt(0) in front of the AGPR reads of the other path: a full drain of the weight ring per pass)
        f32x4 t[16];
        const char *base = reinterpret_cast<const char *>(p.feat + (tc * 8 * 64 + lane) * 8);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const char *a = base + k * 4096;
            asm volatile("global_load_dwordx4 %0, %4, off\n\tglobal_load_dwordx4 %1, %4, off offset:16\n\t"
                         "global_load_dwordx4 %2, %4, off offset:2048\n\tglobal_load_dwordx4 %3, %4, off offset:2064"
                         : "=&v"(t[4 * k]), "=&v"(t[4 * k + 1]), "=&v"(t[4 * k + 2]), "=&v"(t[4 * k + 3]) : "v"(a) : "memory");
        }
        asm volatile("global_load_ubyte %0, %2, off\n\tglobal_load_dword %1, %3, off"
                     : "=&v"(lab), "=&v"(dist) : "v"(p.label + tc * 32 + j), "v"(p.dist + tc * 32 + j) : "memory");
        asm volatile("s_waitcnt vmcnt(0)"
                     : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]), "+v"(t[7]),
                       "+v"(t[8]), "+v"(t[9]), "+v"(t[10]), "+v"(t[11]), "+v"(t[12]), "+v"(t[13]), "+v"(t[14]), "+v"(t[15]),
                       "+v"(lab), "+v"(dist)
                     :: "memory");
        if (!tile_ok) dist = 0.f;
#pragma unroll
        for (int s = 0; s < 8; s++)
#pragma unroll
            for (int e = 0; e < 8; e++) raw[s][e] = t[2 * s + (e >> 2)][e & 3];
    }
#pragma unroll
    for (int s = 0; s < 8; s++) {   // encode_kernel wrote the fragment already split: dwords 0..3 = f16 hi, 4..7 = f16 lo
        const u32x4v hw = {__builtin_bit_cast(unsigned int, raw[s][0]), __builtin_bit_cast(unsigned int, raw[s][1]),
                           __builtin_bit_cast(unsigned int, raw[s][2]), __builtin_bit_cast(unsigned int, raw[s][3])};
        const u32x4v lw = {__builtin_bit_cast(unsigned int, raw[s][4]), __builtin_bit_cast(unsigned int, raw[s][5]),
                           __builtin_bit_cast(unsigned int, raw[s][6]), __builtin_bit_cast(unsigned int, raw[s][7])};
        bh[s] = __builtin_bit_cast(half8, hw);
        bl[s] = __builtin_bit_cast(half8, lw);
    }
}

// input_buffer's partner: step tn of the feature buffer (+ label, dist) -> a[190:255], issued in front of the output layer
__device__ __forceinline__ void input_prefetch(const MlpParams &p, long tn, int lane, int j) {
    const char *base = reinterpret_cast<const char *>(p.feat + ((size_t)tn * 8 * 64 + lane) * 8);
    // k-steps 2k, 2k+1 (2048 B apart), two 16-B halves each -> a[190+16k : 205+16k]
#define SDN_PF_LOAD4(K, R0, R1, R2, R3) \
    asm volatile("global_load_dwordx4 a[" #R0 ":" #R0 "+3], %0, off\n\tglobal_load_dwordx4 a[" #R1 ":" #R1 "+3], %0, off offset:16\n\t" \
                 "global_load_dwordx4 a[" #R2 ":" #R2 "+3], %0, off offset:2048\n\tglobal_load_dwordx4 a[" #R3 ":" #R3 "+3], %0, off offset:2064" \
                 ::"v"(base + (K) * 4096) : "memory", SDN_PF_CLOBBERS)
    // (the clobber list is what makes the kernel's register count include a[190:255])
#define SDN_PF_CLOBBERS "a190", "a191", "a192", "a193", "a194", "a195", "a196", "a197", "a198", "a199", "a200", "a201", "a202", "a203", "a204", "a205", "a206", "a207", "a208", "a209", "a210", "a211", "a212", "a213", "a214", "a215", "a216", "a217", "a218", "a219", "a220", "a221", "a222", "a223", "a224", "a225", "a226", "a227", "a228", "a229", "a230", "a231", "a232", "a233", "a234", "a235", "a236", "a237", "a238", "a239", "a240", "a241", "a242", "a243", "a244", "a245", "a246", "a247", "a248", "a249", "a250", "a251", "a252", "a253"
    SDN_PF_LOAD4(0, 190, 194, 198, 202);
    SDN_PF_LOAD4(1, 206, 210, 214, 218);
    SDN_PF_LOAD4(2, 222, 226, 230, 234);
    SDN_PF_LOAD4(3, 238, 242, 246, 250);
#undef SDN_PF_CLOBBERS
#undef SDN_PF_LOAD4
    asm volatile("global_load_ubyte a254, %0, off" ::"v"(p.label + (size_t)tn * 32 + j) : "memory", "a254");
    asm volatile("global_load_dword a255, %0, off" ::"v"(p.dist + (size_t)tn * 32 + j) : "memory", "a255");
}

// ---- the workgroup's decision words (LDS_FLAGS at LDS address flags_a), accessed with explicit ds instructions: as a `volatile
// int *` they became FLAT loads / stores (sc0 sc1) whose 64-bit addresses hipcc kept in scratch memory and each of which it followed
// with s_waitcnt vmcnt(0) -- a complete drain of the weight ring's DMAs at every group start, after every pass (termination ballot)
// and in every colour-skip decision (seen in the ISA of rounds 4-5: 17 flat operations, 48 of the kernel's 100 B of scratch) ----------
__device__ __forceinline__ void flag_put(unsigned flags_a, int word, int v) {
    asm volatile("ds_write_b32 %0, %1" ::"v"(flags_a + 4u * (unsigned)word), "v"(v) : "memory");
}
__device__ __forceinline__ i32x4v flag_get4(unsigned flags_a, int word0) {     // words word0 .. word0 + 3 (16-byte aligned), landed
    i32x4v f;
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(f) : "v"(flags_a + 4u * (unsigned)word0) : "memory");
    return f;
}
// One workgroup vote: every wave puts `mine` into word word0 + wave, a barrier, everybody reads the four words (the caller reduces
// them, through readfirstlane, so that the decision is provably uniform).  The words may be rewritten only behind a barrier that
// everybody passes after this read.
__device__ __forceinline__ i32x4v workgroup_vote(unsigned flags_a, int word0, int lane, int wave, int mine) {
    if (lane == 0) flag_put(flags_a, word0 + wave, mine);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    return flag_get4(flags_a, word0);
}

// CT = number of split terms of the colour layers fc_5 / fc_6 (3, or 2 = without the Whi.Xlo products)
// FUSED = the encode stage runs inside this kernel (field_kernel): a pass's B fragments, distances and labels come from
//         enc_place / enc_level instead of the feature buffer, the ray flags from the intersections themselves
template <int DBG, int CT, int MODE = MODE_BUFFER>
__global__ __launch_bounds__(256, 1) void mlp_kernel(const MlpParams p) {
    constexpr bool FUSED = MODE == MODE_FUSED || MODE == MODE_FUSED_AUX, AUX = MODE == MODE_FUSED_AUX, RAW = MODE == MODE_RAW;
    // Colour-branch skipping (field_kernel): a sample with relu(sigma) * dist == 0 has volume-rendering weight EXACTLY 0
    // (mc_utils.py:154-161: weights = (1 - exp(-relu(sigma) * dists)) * T), so its colour is multiplied by zero; when that holds
    // for all 128 samples of a workgroup's pass, fc_5 / fc_6 / fc_out_c (35 % of the pass's matrix instructions, 18 of its 46
    // ring slots) are not evaluated at all -- net_out is bit-identical.  sigma is complete only after fc_4's lower half has
    // been activated, which normally happens as fc_5's pending work: sigma_lower_half computes that half's contribution
    // ahead on a copy of the running sum (a few % of a pass), the decision is a wave ballot combined over the 4 waves (they
    // share the weight ring).  (Taking the decision inside fc_5, behind its pending work, costs nothing extra per pass but saves
    // less per skipped pass -- measured on the same box: -4.8 % vs -6.9 % of the kernel time.)
    constexpr bool SKIP = MODE == MODE_FUSED;
    __shared__ __attribute__((aligned(1024))) char lds[LDS_TOTAL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, j = lane & 31;
    const int q = j & 3;

    float *cst = reinterpret_cast<float *>(lds + LDS_CONST);
    stage_consts(cst, p.consts, p.sky_avg);
    // FUSED: the encode stage reads its tables from LDS (a copy of the parameter block with the three pointers redirected)
    EncParams enc = p.enc;
    if constexpr (FUSED)
        stage_enc_tables(enc, p.enc, reinterpret_cast<float *>(lds + LDS_ENC_SCALES), reinterpret_cast<float *>(lds + LDS_ENC_LIN),
                         reinterpret_cast<uint8_t *>(lds + LDS_ENC_LUT), p.cam_ori_dev);
    __syncthreads();

    Ring r;
    r.slots_per_pass = SLOTS_PER_PASS;
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

    // Input prefetch: the next pass's 16 KiB of features (+ label, dist) are loaded into otherwise idle AGPRs while the
    // output layer of the current pass runs, so the HBM latency of the pass-start loads (3.5 % of a pass) is hidden.
    // The loads are inline asm (the compiler would place its own, draining waits) and are consumed only through
    // v_accvgpr_read asm behind a hand-counted wait: after them the output layer always issues its 4 slots x 4 ring
    // DMAs, so "vmcnt(16)" at the next pass start means the prefetch has landed (more vm operations in between -- the
    // stores at a group's end -- only make the wait stricter).
    // The landing registers are the PHYSICAL AGPRs a[190:255], named in the asm text: as C++ values they would be
    // loop-carried, and hipcc keeps loop-carried values in VGPRs, i.e. copies them out of the AGPRs right behind the
    // load -- before the data has landed.  The kernel's own allocation stays below a190 (tools/check_lds_hazards.py
    // verifies that no other instruction touches a[190:255]).
    unsigned t_seg = 0;
    if constexpr (DBG & 512) {
        if (threadIdx.x < 16) reinterpret_cast<unsigned *>(lds + LDS_TIMERS)[threadIdx.x] = 0u;
        t_seg = (unsigned)__builtin_readcyclecounter();
    }
    long pf_tc = -1;            // pass whose inputs sit in a[190:255] (wave-uniform), -1: none
    unsigned long long t_stage = 0, t_kernel0 = 0;
    unsigned n_pass = 0;
    if constexpr (DBG & 128) t_kernel0 = __builtin_readcyclecounter();
    const int n_groups = (p.n_tiles + 3) >> 2;
    // Group schedule.  Static: workgroup b takes groups b, b + G, b + 2G, ... (G = gridDim.x).  With a ticket counter the
    // first TWO rounds are static and every later group is drawn from the counter one group AHEAD of its use (the draw
    // of group n+2 is issued at the start of group n, so the group after the current one is always known: its first pass
    // is prefetched during the current group's last).  Groups are independent, so net_out does not depend on the schedule.
    // (The atomic's round trip IS waited for at the group's start: hipcc consumes an atomic's result at once -- `vmcnt(0)`
    // behind it, once per group, <= 0.6 % of a group's time.  Keeping the draw pending for one more group was tried in
    // round 6: the result is then a loop-carried value, which hipcc copies into its carrier register right behind the
    // atomic, with the same wait; returning it into a reserved physical register is what the AGPR prefetch of the
    // two-kernel form does, and is not worth a second such contract here.)
    const unsigned flags_a = lds_addr(lds + LDS_FLAGS);   // the workgroup's decision words (workgroup_vote)
    int grp = blockIdx.x, grp_next = blockIdx.x + (int)gridDim.x;
    // FUSED: the first intersection of this lane's ray in group g (0 = none / no ray).  The next group's is loaded at the
    // START of the current one, so a group does not begin with an exposed round trip to memory
    auto first_vox = [&](int g) -> int {
        const int t = g * 4 + wave, ry = t * RAYS_PER_TILE + (j >> 2);
        if (!(g < n_groups && t < p.n_tiles && ry < p.R && enc.win.valid(ry))) return 0;
        return enc.voxel_id[(size_t)enc.win.src(ry) * enc.M];
    };
    int vox_cur = 0;
    if constexpr (FUSED) vox_cur = first_vox(grp);
    int cold = 0;     // (uniform) consecutive groups of this workgroup that were found dense, or not asked (colour-branch skipping)
    while (grp < n_groups) {
        const int tile = grp * 4 + wave;
        const bool tile_ok = tile < p.n_tiles;
        const int tile_s = grp * 4 + r.wave;              // the same as scalars (r.wave went through readfirstlane)
        const bool tile_ok_s = tile_s < p.n_tiles;
        const int ray = tile * RAYS_PER_TILE + (j >> 2);
        const bool ray_ok = tile_ok && ray < p.R && (!FUSED || p.win.valid(ray));
        const int rl = ray_ok ? ray : p.R - 1;            // FUSED: local ray / the same ray in the frame-wide arrays
        const int rr = FUSED ? enc.win.src(rl) : 0;
        uint8_t flag;                                      // bit 0 sky_only, bit 1 nosky (FUSED: bit 1 is known at the group's end)
        int vox_nxt = 0;
        if constexpr (FUSED) {
            flag = vox_cur != 0 ? (uint8_t)0 : (uint8_t)1;   // scenedreamer.py:337
            vox_nxt = first_vox(grp_next);
        } else if constexpr (RAW) flag = tile_ok ? (uint8_t)0 : (uint8_t)1;   // every tile holds at least one row
        else flag = ray_ok ? p.rayflag[ray] : (uint8_t)1;
        bool gnd = false;                                  // FUSED: any sample of the ray at world x <= 1 (:380)
        int drawn = grp_next + (int)gridDim.x;            // the group after next: static stride, or ...
        if (p.ticket && threadIdx.x == 0) drawn = 2 * (int)gridDim.x + atomicAdd(p.ticket, 1);   // ... the next undrawn one
        // (AUX also returns the per-sample sigma / colour of rays that hit nothing -- the reference evaluates them -- so it skips no group)
        const bool any_hit = AUX ? tile_ok : __any(!(flag & 1));
        // workgroup-uniform decisions: skip the group when none of its 32 rays hits anything; everybody learns the draw
        if (threadIdx.x == 0) flag_put(flags_a, 4, drawn);
        // readfirstlane makes the decisions provably uniform: otherwise every loop-carried ring counter / pointer is
        // classified divergent, lives in VGPRs (spills!) and the DMA cannot use scalar addressing
        const i32x4v fh = workgroup_vote(flags_a, 0, lane, wave, any_hit ? 1 : 0), fd = flag_get4(flags_a, 4);
        const bool grp_hit = __builtin_amdgcn_readfirstlane(fh[0] | fh[1] | fh[2] | fh[3]) != 0;
        const int grp_next2 = __builtin_amdgcn_readfirstlane(fd[0]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();   // the next group rewrites the flags only after everyone has read them

        float outq[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        float carry = 0.f, tsum = 0.f;
        int n_done = 0, n_colour = 0;
        // (uniform) whether the next pass of this group takes the colour-skip decision at all.  Across groups: after 6 groups in a row
        // whose first pass was less than 1/4 empty (a field with surfaces: rays saturate, nothing is empty) only every 4th group
        // still decides -- there the early sigma was +1 % of the frame for nothing (tools/bench_opaque.py); on the benchmark
        // frames the rule costs about one point of skipped passes (dense stretches end somewhere)
        bool skip_test = SKIP && !p.no_colour_skip && (cold < 6 || (cold & 3) == 0);
        if (SKIP && !skip_test) cold++;

        for (int ch = 0; grp_hit && ch < p.nch; ch++) {
            const size_t tc = (size_t)(tile_ok ? tile : 0) * p.nch + ch;
            half8 bh[16], bl[16];
            f32x16 acc[8];
            MxState mx;
            if constexpr (CT == 6) {
#pragma unroll
                for (int k = 0; k < 4; k++) mx.bm[k] = 0.f;
            }
            seg_tick<DBG>(lds, 9, t_seg);
            unsigned long long t_in0 = 0;
            if constexpr (DBG & 128) t_in0 = __builtin_readcyclecounter();
            const long tc_s = (long)(tile_ok_s ? tile_s : 0) * p.nch + ch;    // tc as a scalar
            // ---- input stage: this pass's B fragments (f16 hi / lo) and every sample's label and distance --------------------------
            int lab;
            float dist;
            float smp_depth = 0.f;   // AUX: this lane's sample depth
            // RAW: this lane's row of the [R, 128] feature matrix
            const long row = (long)(tile_ok ? tile : 0) * 256 + ch * 32 + j;
            if constexpr (RAW) {   // (inline: as a function of its own this loop costs mlp_kernel<0, 6, RAW> two VGPR spills)
                const long rc = row < p.R ? row : (long)p.R - 1;   // clamped: lanes past the end evaluate the last row, store nothing
                lab = p.label[rc];
                dist = 0.f;
                const float *src = p.feat + rc * FEAT + 8 * h;   // kmap_first: k-step s, lane half h = features 16 s + 8 h .. + 7
#pragma unroll
                for (int s = 0; s < 8; s++) {
                    const float4 a = *reinterpret_cast<const float4 *>(src + 16 * s), b = *reinterpret_cast<const float4 *>(src + 16 * s + 4);
                    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                    split8(v, bh[s], bl[s]);
                }
            }
            else if constexpr (FUSED)
                input_encode(enc, rr, rl, ch * SAMP_PER_STEP + (j & 3), ray_ok, AUX ? ray_ok : !(flag & 1), h, bh, bl, lab, dist, gnd, smp_depth);
            else input_buffer<DBG>(p, tc, pf_tc == tc_s && !(DBG & 256), tile_ok, lane, j, bh, bl, lab, dist);
            if constexpr (DBG & 128) {
                asm volatile("s_waitcnt vmcnt(0)" ::"v"(bh[7]), "v"(bl[7]) : "memory");
                t_stage += __builtin_readcyclecounter() - t_in0;
                n_pass++;
            }
            if constexpr (DBG & 512) asm volatile("s_waitcnt vmcnt(0)" ::"v"(bh[7]), "v"(bl[7]) : "memory");
            seg_tick<DBG>(lds, 0, t_seg);
            float part = 0.f;
            bool colour_skipped = false;
            const float *wsig = cst + C_WSIGMA;
            // ---- fc_1: 8 k-steps; fragments 0..6 of its upper half are activated behind its own lower half, fragment 7
            //      right after it, its lower half behind fc_2's head ---------------------------------------------------
            const float *bias1 = cst + C_LABEL_BIAS + lab * HID;
            layer8<DBG, 8, false, false, false>(lds, r, bh, bl, acc, bias1, bias1, wsig, h, part, TRUNK_K, TRUNK_K);
            act_step<7, false>(acc, bias1, wsig, h, bh, bl, part, TRUNK_K);   // fragments 0..6 were activated inside the layer
            seg_tick<DBG>(lds, 1, t_seg);
            // ---- fc_2 .. fc_6.  fc_4 (l == 2) feeds the density head (layers.py:114): its upper half is activated
            //      inside l == 2, its lower half as the pending work of l == 3 ----------------------------------------
#pragma unroll 1
            for (int l = 0; l < 5; l++) {   // (straight-line code instead of this loop: 1.5 KB of scratch spills -- tried)
                const float *bias = cst + C_BETA + l * HID;
                const float *bias_pend = l == 0 ? bias1 : bias - HID;   // the previous layer's (its lower half is pending)
                // the trunk's packed weights carry 2^TRUNK_SHIFT (pack_kernel): its accumulators are descaled in the bias fma.
                // (this layer is fc_(l+2), the pending one fc_(l+1); literals per branch -- as run-time scalars they cost spills)
                constexpr float tk = TRUNK_K;
                if constexpr (CT == 6) {   // colour layers: f16 Whi.Xhi + fp6 corrections (layer8x)
                    if (l == 2) layer8x<DBG, 0, false, true>(lds, r, bh, bl, mx, acc, bias, bias_pend, wsig, h, part, tk, tk);
                    else if (l == 3) layer8x<DBG, 1, true, false>(lds, r, bh, bl, mx, acc, bias, bias_pend, wsig, h, part, 1.f, tk);
                    else if (l == 4) layer8x<DBG, 2, false, false>(lds, r, bh, bl, mx, acc, bias, bias_pend, wsig, h, part, 1.f, 1.f);
                    else layer8<DBG, 16, true, false, false>(lds, r, bh, bl, acc, bias, bias_pend, wsig, h, part, tk, tk);
                } else {
                    // fc_4's upper half feeds fc_5, fc_5's activations feed fc_5 / fc_6: no lo parts when those are 2-term
                    if (l == 2) layer8<DBG, 16, true, false, true, 3, true, CT == 3>(lds, r, bh, bl, acc, bias, bias_pend, wsig, h, part, tk, tk);
                    else if (l == 3) layer8<DBG, 16, true, true, false, CT, CT == 3, CT == 3>(lds, r, bh, bl, acc, bias, bias_pend, wsig, h, part, 1.f, tk);
                    else if (CT != 3 && l == 4) layer8<DBG, 16, true, false, false, CT, CT == 3, true>(lds, r, bh, bl, acc, bias, bias_pend, wsig, h, part, 1.f, 1.f);
                    else if (l == 4) layer8<DBG, 16, true, false, false>(lds, r, bh, bl, acc, bias, bias_pend, wsig, h, part, 1.f, 1.f);
                    else layer8<DBG, 16, true, false, false>(lds, r, bh, bl, acc, bias, bias_pend, wsig, h, part, tk, tk);
                }
                seg_tick<DBG>(lds, 2 + l, t_seg);
                if constexpr (SKIP) {
                    if (l == 2 && skip_test) {
                        // sigma of this pass: `part` holds fc_4's upper half, the lower half's terms are added on a copy (fc_5's
                        // pending work adds them to `part` itself, in the same order, if the pass goes on)
                        float part_e = part;
                        sigma_lower_half(std::make_integer_sequence<int, 16>{}, acc, bias, wsig, h, bh, bl, part_e, tk);
                        const float sigma_e = part_e + __shfl_xor(part_e, 32) + cst[C_BSIGMA];
                        const bool zero_w = !ray_ok || (flag & 1) || fmaxf(sigma_e, 0.f) * dist == 0.f;
                        const int wave_zero = __popcll(__ballot(zero_w));          // lanes: 2 per sample
                        // ONE barrier: flags[8..11] are written only here, and a wave reaches its next write only through the ring
                        // barriers of at least one whole layer, which nobody passes before having read these
                        const i32x4v fz = workgroup_vote(flags_a, 8, lane, wave, wave_zero);
                        const int grp_zero = __builtin_amdgcn_readfirstlane(fz[0] + fz[1] + fz[2] + fz[3]);
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        seg_tick<DBG>(lds, 11, t_seg);
                        // Whether a pass is empty hardly depends on the depth along the rays (measured on the benchmark frames,
                        // tools/dbg_sigma_stats.py: P(next pass of the group empty | this one empty) = 0.89 - 0.93, | this one less
                        // than 3/4 empty: 0.000 - 0.002), so a group stops taking the decision -- the work of computing sigma
                        // ahead -- after a pass that was not at least 3/4 empty.  Purely a cost heuristic: net_out cannot change.
                        // (Tried on top: a WAVE whose own 32 samples are empty sitting the colour layers out while the others work --
                        //  barriers and its share of the ring DMA only.  Same box: 15.03 -> 15.55 ms, 18.49 -> 19.08 ms: the idle
                        //  SIMD buys the other three nothing, the extra decisions cost.  Not kept.)
                        skip_test = grp_zero >= 192;
                        if (ch == 0) cold = grp_zero < 64 ? cold + 1 : 0;
                        if (grp_zero == 256) { colour_skipped = true; break; }
                    }
                }
            }
            if constexpr (SKIP) {
                if (colour_skipped) {
                    // every weight of the pass is exactly zero: carry, tsum and outq would all be incremented by +0
                    ring_restart(lds, r);
                    if constexpr (DBG & 512) {
                        if (threadIdx.x == 0) {
                            reinterpret_cast<unsigned *>(lds + LDS_TIMERS)[10] += 1u;
                            reinterpret_cast<unsigned *>(lds + LDS_TIMERS)[12] += 1u;
                        }
                    }
                    n_done = ch + 1;
                    continue;   // (no termination ballot: the transmittances did not change since the last one)
                }
            }
            n_colour++;
            // ---- fc_out_c ------------------------------------------------------------------------------------------
            {   // inputs of the next pass of this wave: the next step of this tile, or the first step of its next group
                long tn = tc_s + 1;
                bool has_next = tile_ok_s;
                if (ch + 1 == p.nch) {
                    // first step of this wave's tile in the workgroup's next group (wasted if that group hits nothing)
                    const int tile2 = grp_next * 4 + r.wave;
                    has_next = tile2 < p.n_tiles;
                    tn = (long)tile2 * p.nch;
                }
                pf_tc = -1;
                if (MODE == MODE_BUFFER && has_next && !(DBG & 256)) {
                    pf_tc = tn;
                    input_prefetch(p, tn, lane, j);
                }
            }
            f32x16 col[2];
            col[0] = bias_block<0>(cst + C_BC, h);
            col[1] = bias_block<1>(cst + C_BC, h);
            layer_out<DBG>(lds, r, bh, bl, acc, col, cst + C_BETA + 4 * HID, h, part);
            seg_tick<DBG>(lds, 7, t_seg);
            const float sigma = part + __shfl_xor(part, 32) + cst[C_BSIGMA];
            if constexpr (RAW) {   // LightningMLP.forward's outputs for this lane's row: (sigma, c), layers.py:114, :124
                if (tile_ok && row < p.R) {
                    if (h == 0) p.sigma_out[row] = sigma;
                    store_colour_row(p.net_out + (size_t)row * OUTC, col, h);
                }
                n_done = ch + 1;
                continue;
            }
            // ---- volume rendering + this pass's share of the ray's colour (field_composite.h) ----------------------
            const float wgt = render_weight(sigma, dist, q, carry);
            tsum += wgt;
            if constexpr (AUX) {   // the per-sample return values of Generator._forward_perpix
                const int sidx = ch * SAMP_PER_STEP + q;
                if (ray_ok && sidx < p.ns) {
                    const size_t smp = (size_t)p.win.out_row(ray) * p.ns + sidx;
                    if (h == 0) {
                        if (p.w_out) p.w_out[smp] = (flag & 1) ? 0.f : wgt;
                        if (p.depth_out) p.depth_out[smp] = smp_depth;
                        if (p.sig_out) p.sig_out[smp] = sigma;
                    }
                    if (p.col_out) store_colour_row(p.col_out + smp * OUTC, col, h);
                }
            }
            accumulate_colour(col, wgt, q, outq);
            // ---- early ray termination (north star: wavefront ballots): once the transmittance exp(-carry) of EVERY ray of
            //      the workgroup's 32 is below eps, the remaining samples can change net_out by at most 2 eps (their weights
            //      sum to < eps and that mass goes to the sky term instead): skip the group's remaining passes.  The
            //      decision is a wave ballot combined over the 4 waves, because they share the weight ring / barriers.
            if constexpr (DBG & 512) {
                asm volatile("" ::"v"(outq[0][0]), "v"(outq[1][3]), "v"(carry), "v"(tsum));
                seg_tick<DBG>(lds, 8, t_seg);
                if (threadIdx.x == 0) reinterpret_cast<unsigned *>(lds + LDS_TIMERS)[10] += 1u;
            }
            n_done = ch + 1;
            if (p.term_depth > 0.f && ch + 1 < p.nch) {
                const bool opaque = !ray_ok || (flag & 1) || carry > p.term_depth;
                const bool wave_done = __all(opaque);
                const i32x4v ft = workgroup_vote(flags_a, 0, lane, wave, wave_done ? 1 : 0);
                const bool grp_done = __builtin_amdgcn_readfirstlane(ft[0] & ft[1] & ft[2] & ft[3]) != 0;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                if (grp_done) break;
            }
        }
#ifndef SDN_NO_TERM_GND   // (A/B switch for timing the main loop without this cold block; never set for a product build)
        if constexpr (FUSED) {
            // early termination dropped the group's remaining passes: their samples still take part in `is_gnd` (any sample of
            // the ray at world x <= 1, scenedreamer.py:380-382), as they do in encode_kernel -- place them (no gathers, no MLP)
            if (grp_hit && n_done < p.nch) {
                RayBoxes rb;
                float dd[3];
                enc_load_ray(enc, rr, rb, dd);
#pragma unroll 1
                for (int c2 = n_done; c2 < p.nch; c2++)
                    gnd = gnd || enc_place(enc, rb, dd, rl, c2 * SAMP_PER_STEP + (j & 3), ray_ok).gnd;
            }
        }
#endif
        if (p.passes && threadIdx.x == 0) p.passes[grp] = (uint8_t)n_done;   // passes this group went through (tests / bench)
        if (p.colour_passes && threadIdx.x == 0) p.colour_passes[grp] = (uint8_t)n_colour;   // ... and how many of them ran the colour branch

        // ---- blend the sky, store ---------------------------------------------------------------------------------
        if constexpr (!RAW) {
            if constexpr (FUSED) {   // nosky = the ray's last intersection is a voxel, or one of its samples lies at world x <= 1 (:335, :382)
                const int g = quad_any(gnd);
                const bool last_hit = ray_ok && enc.voxel_id[(size_t)rr * enc.M + (enc.M - 1)] != 0;
                if (last_hit || g) flag |= 2;
            }
            blend_sky_store<AUX>(cst, p.sky_c, p.net_out, p.win.src(ray), p.win.out_row(ray), ray_ok, tsum, flag, outq, q, h,
                                 p.skyb_out, p.nosky_out);
        }
        grp = grp_next;
        grp_next = grp_next2;
        vox_cur = vox_nxt;
    }
    // the ring runs DMA_AHEAD slots ahead of the last pass: let it land before the LDS is released
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // the last workgroup to leave resets the ticket counter for the next launch
    if (p.ticket && threadIdx.x == 0 && atomicAdd(p.ticket + 1, 1) == (int)gridDim.x - 1) {
        p.ticket[0] = 0;
        p.ticket[1] = 0;
    }
    if constexpr (DBG & 512) {   // per-segment cycles of this workgroup's thread 0 into its first net_out row (floats 3..13)
        __syncthreads();
        if (threadIdx.x < 13) p.net_out[(size_t)(blockIdx.x * 4) * OUTC + 3 + threadIdx.x] = (float)reinterpret_cast<unsigned *>(lds + LDS_TIMERS)[threadIdx.x];
    }
    if constexpr (DBG & 128) {   // timing experiment: (input-staging cycles, total cycles, passes) of this wave into net_out
        if (lane == 0) {
            float *o = p.net_out + (size_t)(blockIdx.x * 4 + wave) * OUTC;
            o[0] = (float)t_stage; o[1] = (float)(__builtin_readcyclecounter() - t_kernel0); o[2] = (float)n_pass;
        }
    }
}

// =====================================================================================================
// debug probe: checks the MFMA operand layouts the layer machinery relies on (tests/test_fused_gpu.py)
// =====================================================================================================
__global__ void mfma_probe_kernel(const float *A, const float *B, float *C) {
    // A [32][16], B [16][32] row-major fp32 -> C [32][32]
    const int lane = threadIdx.x, h = lane >> 5, j = lane & 31;
    half8 a, b;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        a[e] = (_Float16)A[j * 16 + 8 * h + e];
        b[e] = (_Float16)B[(8 * h + e) * 32 + j];
    }
    f32x16 c;
#pragma unroll
    for (int r = 0; r < 16; r++) c[r] = 0.f;
    c = mfma16(a, b, c);
#pragma unroll
    for (int r = 0; r < 16; r++) C[((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + j] = c[r];
}

}  // namespace

// =====================================================================================================
// C ABI
// =====================================================================================================
extern "C" {

size_t sdn_field_consts_floats(void) { return C_TOTAL; }
int sdn_field_const_offset(int which) {
    switch (which) {
        case 0: return C_LABEL_BIAS;
        case 1: return C_BETA;
        case 2: return C_WSIGMA;
        case 3: return C_BC;
        case 4: return C_BSIGMA;
        case 5: return C_SKY_AVG;
        default: return -1;
    }
}

int sdn_field_collapse_table(const float *embeddings, const int32_t *offsets_host, uint32_t L, float S, uint32_t H,
                             const float *genc_host, float *table3, sdn_stream_t stream) {
    SDN_REQUIRE(embeddings && offsets_host && genc_host && table3, "sdn_field_collapse_table: null pointer");
    if (L != NLEV) return sdn::fail(SDN_ERR_UNSUPPORTED, "fused field path needs the 16-level SceneDreamer grid");
    CollapseParams p;
    p.emb = embeddings;
    p.table3 = table3;
    const uint32_t T = (uint32_t)(offsets_host[1] - offsets_host[0]);
    if (T == 0 || (T & (T - 1)) != 0)
        return sdn::fail(SDN_ERR_UNSUPPORTED, "fused field path needs a power-of-two hash table per level");
    p.T = T;
    for (uint32_t l = 0; l < L; l++) {
        if ((uint32_t)(offsets_host[l + 1] - offsets_host[l]) != T)
            return sdn::fail(SDN_ERR_UNSUPPORTED, "fused field path needs equally sized levels");
        const float scale = exp2f((float)l * S) * (float)H - 1.0f;
        const uint32_t res = (uint32_t)ceilf(scale) + 1;
        // every level must take the hash branch of get_grid_index (gridencoder.cu:60-69) on the 5-D grid
        double stride = 1;
        for (int d = 0; d < 5 && stride <= (double)T; d++) stride *= (double)(res + 1);
        if (!(stride > (double)T))
            return sdn::fail(SDN_ERR_UNSUPPORTED, "fused field path needs every level hashed (level %u is dense)", l);
        p.off[l] = (uint32_t)offsets_host[l];
        float fr[2];
        uint32_t pg[2];
        for (int d = 0; d < 2; d++) {
            const float x = (genc_host[d] + 1.f) / 2.f;  // grid.py:144
            volatile float prod = x * scale;             // two roundings, like the kernels
            const float pos = prod + 0.5f;
            const float fl = floorf(pos);
            pg[d] = (uint32_t)fl;
            fr[d] = pos - fl;
        }
        for (int c = 0; c < 4; c++) {
            const int c3 = c & 1, c4 = c >> 1;
            const uint32_t k = ((pg[0] + c3) * 3674653429u) ^ ((pg[1] + c4) * 2097192037u);
            p.K[l][c] = k & (T - 1);
            // reference multiply order: ((((1*w0)*w1)*w2)*w3)*w4 -> here the trailing w3*w4 factor
            volatile float w3 = c3 ? fr[0] : 1.f - fr[0];
            volatile float w4 = c4 ? fr[1] : 1.f - fr[1];
            p.w[l][c] = w3 * w4;
        }
    }
    hipLaunchKernelGGL(collapse_kernel, dim3(sdn::div_up<uint32_t>(T, 256), L), dim3(256), 0, (hipStream_t)stream, p);
    return sdn::check_launch("sdn_field_collapse_table");
}

size_t sdn_field_feat_bytes(int32_t n_rays, int32_t num_samples) {
    const size_t tiles = (size_t)sdn::div_up(n_rays, RAYS_PER_TILE), nch = (size_t)sdn::div_up(num_samples, SAMP_PER_STEP);
    return tiles * nch * 8 * 64 * 8 * sizeof(float);
}
size_t sdn_field_aux_elems(int32_t n_rays, int32_t num_samples) {
    const size_t tiles = (size_t)sdn::div_up(n_rays, RAYS_PER_TILE), nch = (size_t)sdn::div_up(num_samples, SAMP_PER_STEP);
    return tiles * nch * 32;
}


int sdn_field_encode(const int32_t *voxel_id, const float *depth2, const float *raydirs, const uint8_t *lut1024,
                     const float *table3, uint32_t table_rows, const float *scales_dev, const float *genc_host,
                     const float *cam_ori_host, const float *voxel_dims_host, const float *lin_dev, const float *u_dev,
                     int32_t n_rays, int32_t max_blocks, int32_t num_samples, float sample_depth, float dists_scale, float *feat,
                     float *dist, uint8_t *label, uint8_t *rayflag, const int32_t *window_host, int32_t strat_division,
                     sdn_stream_t stream) {
    SDN_REQUIRE(feat && dist && label && rayflag, "sdn_field_encode: null pointer");
    EncParams p;
    if (int rc = fill_enc(p, "sdn_field_encode", voxel_id, depth2, raydirs, lut1024, table3, table_rows, scales_dev, genc_host, cam_ori_host,
                          voxel_dims_host, lin_dev, u_dev, n_rays, max_blocks, num_samples, sample_depth, dists_scale, strat_division))
        return rc;
    p.feat = feat; p.dist = dist; p.label = label; p.rayflag = rayflag;
    if (int rc = set_window(p.win, window_host, n_rays, "sdn_field_encode")) return rc;
    hipLaunchKernelGGL(encode_kernel, dim3(sdn::div_up(p.n_tiles, 4)), dim3(256), 0, (hipStream_t)stream, p);
    return sdn::check_launch("sdn_field_encode");
}

int sdn_sample_depth(const float *depth2, const float *lin_dev, const float *u_dev, int32_t n_rays, int32_t max_blocks,
                     int32_t n_points, float sample_depth, float *rand_depth, float *new_dists, int64_t *idx,
                     int32_t strat_division, sdn_stream_t stream) {
    SDN_REQUIRE(depth2 && lin_dev && rand_depth && new_dists && idx, "sdn_sample_depth: null pointer");
    SDN_REQUIRE(strat_division == 0 || strat_division == 1, "sdn_sample_depth: strat_division must be 0 (x * (1/n)) or 1 (x / n)");
    SDN_REQUIRE(n_rays > 0 && n_points >= 2, "sdn_sample_depth: need at least one ray and two stratified points");
    if (max_blocks < 1 || max_blocks > MAXM) return sdn::fail(SDN_ERR_UNSUPPORTED, "sdn_sample_depth: max_blocks must be 1..8");
    SampleParams p;
    p.depth2 = depth2; p.lin = lin_dev; p.u = u_dev; p.rand_depth = rand_depth; p.new_dists = new_dists; p.idx = idx;
    p.R = n_rays; p.M = max_blocks; p.n_points = n_points; p.sample_depth = sample_depth; p.ieee_div = strat_division;
    hipLaunchKernelGGL(sample_depth_kernel, dim3(sdn::div_up(n_rays, 256)), dim3(256), 0, (hipStream_t)stream, p);
    return sdn::check_launch("sdn_sample_depth");
}

static int fill_mlp(MlpParams &p, const char *who, const void *packed, const float *consts, const float *sky_c, float *net_out,
                    int32_t n_rays, int32_t num_samples, int32_t colour_terms, float term_eps, uint8_t *passes, const int32_t *window_host,
                    const float *sky_avg, int32_t *ticket, int32_t *launch_rays = nullptr) {
    if (!(packed && consts && sky_c && net_out)) return sdn::fail(SDN_ERR_INVALID, "%s: null pointer", who);
    if (!(n_rays > 0 && num_samples > 0)) return sdn::fail(SDN_ERR_INVALID, "%s: empty frame", who);
    if (!(colour_terms == 2 || colour_terms == 3 || colour_terms == 6)) return sdn::fail(SDN_ERR_INVALID, "%s: colour_terms must be 2, 3 or 6", who);
    if (!(term_eps >= 0.f && term_eps < 1.f)) return sdn::fail(SDN_ERR_INVALID, "%s: term_eps must be in [0, 1)", who);
    p.term_depth = term_eps > 0.f ? -logf(term_eps) : 0.f;
    p.passes = passes;
    p.wpk = (const half8 *)packed;
    p.consts = consts; p.sky_c = sky_c; p.net_out = net_out;
    p.sky_avg = sky_avg; p.ticket = ticket;
    if (int rc = set_window(p.win, window_host, n_rays, who, launch_rays)) return rc;
    p.R = n_rays; p.ns = num_samples;
    p.nch = sdn::div_up(num_samples, SAMP_PER_STEP);
    p.n_tiles = sdn::div_up(n_rays, RAYS_PER_TILE);
    return 0;
}

int sdn_field_mlp(const float *feat, const float *dist, const uint8_t *label, const uint8_t *rayflag, const void *packed,
                  const float *consts, const float *sky_c, float *net_out, int32_t n_rays, int32_t num_samples,
                  int32_t colour_terms, float term_eps, uint8_t *passes, int32_t n_workgroups, const int32_t *window_host,
                  const float *sky_avg, int32_t *ticket, sdn_stream_t stream) {
    SDN_REQUIRE(feat && dist && label && rayflag, "sdn_field_mlp: null pointer");
    MlpParams p{};
    if (int rc = fill_mlp(p, "sdn_field_mlp", packed, consts, sky_c, net_out, n_rays, num_samples, colour_terms, term_eps, passes, window_host,
                          sky_avg, ticket))
        return rc;
    p.feat = feat; p.dist = dist; p.label = label; p.rayflag = rayflag;
    const int wg = field_workgroups(p.n_tiles, n_workgroups);
    static const int dbg = [] {
        const char *e = getenv("SDN_MLP_DBG");   // timing experiments only; results are wrong unless 0
        return e ? atoi(e) : 0;
    }();
    switch (dbg) {
#ifdef SDN_MLP_ABLATION
        case 1: hipLaunchKernelGGL((mlp_kernel<1, 3>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); break;   // no ring DMA
        case 256: hipLaunchKernelGGL((mlp_kernel<256, 3>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); break; // no input prefetch
        case 384: hipLaunchKernelGGL((mlp_kernel<384, 3>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); break;
        case 128: hipLaunchKernelGGL((mlp_kernel<128, 3>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); break; // input-staging timer
        case 2: hipLaunchKernelGGL((mlp_kernel<2, 3>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); break;   // no ring barrier
        case 3: hipLaunchKernelGGL((mlp_kernel<3, 3>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); break;
        case 4: hipLaunchKernelGGL((mlp_kernel<4, 3>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); break;   // no activation VALU
        case 8: hipLaunchKernelGGL((mlp_kernel<8, 3>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); break;   // no fragment ds_read
        case 16: hipLaunchKernelGGL((mlp_kernel<16, 3>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); break; // no MFMA
        case 28: hipLaunchKernelGGL((mlp_kernel<28, 3>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); break;
        case 32: hipLaunchKernelGGL((mlp_kernel<32, 6>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); break;  // colour layers without Wlo.X
        case 64: hipLaunchKernelGGL((mlp_kernel<64, 6>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); break;  // ... without Whi.Xlo
        case 96: hipLaunchKernelGGL((mlp_kernel<96, 6>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); break;  // ... Whi.Xhi only
        case 512: hipLaunchKernelGGL((mlp_kernel<512, 6>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); break; // per-segment timers
        case 515: hipLaunchKernelGGL((mlp_kernel<512, 3>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); break;
        case 513: hipLaunchKernelGGL((mlp_kernel<513, 6>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); break; // timers + one ablation
        case 514: hipLaunchKernelGGL((mlp_kernel<514, 6>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); break;
        case 516: hipLaunchKernelGGL((mlp_kernel<516, 6>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); break;
        case 520: hipLaunchKernelGGL((mlp_kernel<520, 6>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); break;
#endif
        default:
            if (colour_terms == 2) hipLaunchKernelGGL((mlp_kernel<0, 2>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p);
            else if (colour_terms == 6) hipLaunchKernelGGL((mlp_kernel<0, 6>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p);
            else hipLaunchKernelGGL((mlp_kernel<0, 3>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p);
            break;
    }
    return sdn::check_launch("sdn_field_mlp");
}

int sdn_field_render(const int32_t *voxel_id, const float *depth2, const float *raydirs, const uint8_t *lut1024, const float *table3,
                     uint32_t table_rows, const float *scales_dev, const float *genc_host, const float *cam_ori_host,
                     const float *voxel_dims_host, const float *lin_dev, const float *u_dev, int32_t n_rays, int32_t max_blocks,
                     int32_t num_samples, float sample_depth, float dists_scale, const void *packed, const float *consts,
                     const float *sky_c, const float *sky_avg, float *net_out, int32_t colour_terms, float term_eps, uint8_t *passes,
                     int32_t n_workgroups, const int32_t *window_host, int32_t strat_division, int32_t *ticket, const float *cam_ori_dev,
                     const sdn_field_aux *aux, sdn_stream_t stream) {
    MlpParams p{};
    const bool want_aux = aux && (aux->weights || aux->depth || aux->sigma || aux->colour || aux->sky_blended || aux->nosky);
    SDN_REQUIRE(!(want_aux && term_eps > 0.f), "sdn_field_render: the per-sample outputs need term_eps = 0 (every pass must run)");
    static const float zero3[3] = {0.f, 0.f, 0.f};
    if (cam_ori_dev && !cam_ori_host) cam_ori_host = zero3;
    int32_t launch_rays = n_rays;
    if (int rc = fill_mlp(p, "sdn_field_render", packed, consts, sky_c, net_out, n_rays, num_samples, colour_terms, term_eps, passes,
                          window_host, sky_avg, ticket, &launch_rays))
        return rc;
    if (int rc = fill_enc(p.enc, "sdn_field_render", voxel_id, depth2, raydirs, lut1024, table3, table_rows, scales_dev, genc_host,
                          cam_ori_host, voxel_dims_host, lin_dev, u_dev, n_rays, max_blocks, num_samples, sample_depth, dists_scale,
                          strat_division))
        return rc;
    p.enc.win = p.win;
    if (launch_rays != n_rays) {   // ragged blocked window: the launch walks the whole block grid (the extra positions are no rays)
        SDN_REQUIRE(u_dev == nullptr, "sdn_field_render: stochastic sampling with the ragged blocked order is not supported");
        p.R = p.enc.R = launch_rays;
        p.n_tiles = p.enc.n_tiles = launch_rays / RAYS_PER_TILE;
    }
    p.cam_ori_dev = cam_ori_dev;
    if (want_aux) {
        p.w_out = aux->weights; p.depth_out = aux->depth; p.sig_out = aux->sigma; p.col_out = aux->colour;
        p.skyb_out = aux->sky_blended; p.nosky_out = aux->nosky;
    }
    if (aux) {   // (these two do not select the per-sample-output instantiation)
        p.colour_passes = aux->colour_passes;
        p.no_colour_skip = (aux->flags & SDN_FIELD_NO_COLOUR_SKIP) ? 1 : 0;
    }
    SDN_REQUIRE(colour_terms != 2, "sdn_field_render: colour_terms must be 3 or 6 (the 2-term profile exists for sdn_field_mlp only)");
    const int wg = field_workgroups(p.n_tiles, n_workgroups);
#ifdef SDN_MLP_ABLATION
    if (const char *e = getenv("SDN_MLP_DBG")) {   // timing experiments only
        if (atoi(e) == 512) { hipLaunchKernelGGL((mlp_kernel<512, 6, MODE_FUSED>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); return sdn::check_launch("sdn_field_render"); }
        if (atoi(e) == 515) { hipLaunchKernelGGL((mlp_kernel<512, 3, MODE_FUSED>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p); return sdn::check_launch("sdn_field_render"); }
    }
#endif
    if (want_aux) {
        if (colour_terms == 6) hipLaunchKernelGGL((mlp_kernel<0, 6, MODE_FUSED_AUX>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((mlp_kernel<0, 3, MODE_FUSED_AUX>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p);
    } else if (colour_terms == 6) hipLaunchKernelGGL((mlp_kernel<0, 6, MODE_FUSED>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((mlp_kernel<0, 3, MODE_FUSED>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p);
    return sdn::check_launch("sdn_field_render");
}

// LightningMLP.forward as an op (imaginaire/model_utils/layers.py:92-126, N = 1 so the ModLinear modulation is folded into
// the packed weights / consts exactly as for sdn_field_render)
int sdn_render_mlp(const float *x, const uint8_t *label, const void *packed, const float *consts, float *sigma, float *c,
                   int64_t n_rows, int32_t colour_terms, int32_t n_workgroups, int32_t *ticket, sdn_stream_t stream) {
    SDN_REQUIRE(x && label && packed && consts && sigma && c, "sdn_render_mlp: null pointer");
    SDN_REQUIRE(n_rows > 0 && n_rows < ((int64_t)1 << 31), "sdn_render_mlp: n_rows must be in [1, 2^31)");
    SDN_REQUIRE(colour_terms == 3 || colour_terms == 6, "sdn_render_mlp: colour_terms must be 3 or 6");
    MlpParams p{};
    p.feat = x; p.label = label;
    p.wpk = (const half8 *)packed; p.consts = consts; p.net_out = c;
    p.R = (int32_t)n_rows; p.ns = 32; p.nch = 8;
    p.n_tiles = (int32_t)((n_rows + 255) / 256);
    p.win = raw_window(p.R);
    p.ticket = ticket;
    p.sigma_out = sigma;
    const int wg = field_workgroups(p.n_tiles, n_workgroups);
    if (colour_terms == 6) hipLaunchKernelGGL((mlp_kernel<0, 6, MODE_RAW>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((mlp_kernel<0, 3, MODE_RAW>), dim3(wg), dim3(256), 0, (hipStream_t)stream, p);
    return sdn::check_launch("sdn_render_mlp");
}

int sdn_debug_mfma_probe(const float *A, const float *B, float *C, sdn_stream_t stream) {
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, A, B, C);
    return sdn::check_launch("sdn_debug_mfma_probe");
}

}  // extern "C"

