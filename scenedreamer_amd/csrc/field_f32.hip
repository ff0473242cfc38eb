// The field in plain fp32 on the f32-input matrix instruction of gfx950 (v_mfma_f32_32x32x2_f32): sample placement ->
// hash-grid lookup -> LightningMLP -> volume rendering + sky compositing, and LightningMLP.forward as an op of its own.
// Replaces Generator._forward_perpix / _forward_perpix_sub (imaginaire/generators/scenedreamer.py:285-430) with
// LightningMLP.forward (imaginaire/model_utils/layers.py:92-126) and volum_rendering_relu (mc_utils.py:154-161), like
// field.hip -- but every product is an f32 x f32 fmaf: the MFMA result is bit for bit a k-ordered fmaf chain, so the
// weights have fp32's RANGE (no 2^8-scaled f16 stream, no TrunkRangeError) and the path needs no calibration gate.  What it
// does NOT buy is accuracy on in-range weights: the 3-term f16 split of field.hip is already as close to fp64 as fp32 is.
// At 1/16 of the f16 MFMA rate it is the fallback rung for styles the f16 kernels cannot serve, not the default.
//
//   field_f32_kernel<FIELD>   per 32-sample tile (8 rays x 4 samples per wave, 4 waves = a 32-ray group per workgroup): the
//                             encode stage of field_kernel (the same device functions, field_enc.h), fc_1 + label bias ->
//                             fc_2 .. fc_4 -> fc_sigma, fc_5, fc_6, fc_out_c, then the compositing epilogue mlp_kernel runs too
//                             (field_composite.h: ONE definition of the volume rendering and the sky blend).  Every sample
//                             of every ray that hits something is evaluated: no early termination, no colour-branch skipping.
//   field_f32_kernel<FIELD_AUX>  the same, plus the other return values of Generator._forward_perpix (scenedreamer.py:429-430) per
//                             sample -- weights, rand_depth, net_out_s, net_out_c -- and per ray -- the blended sky features, nosky_mask --
//                             like field.hip's MODE_FUSED_AUX: no group is skipped and rays that hit nothing are gathered too (the
//                             reference evaluates them).
//   field_f32_kernel<RAW>     rows x [n,128] + label u8 [n] -> sigma [n], c [n,64].
//   pack_f32_kernel           the folded weights in the order the kernel consumes them.
//
// Lanes, streams and the chunk pipeline are mlp_f32.h's (the one statement of the layout).  What is the field's own: the encode stage
// feeds fc_1 the way a layer feeds the next -- lane (h, j) blends levels 2 s + h, k-step (s, c) takes channel c of that level from
// it -- and the stream is 46 chunks per pass (4 fc_1, 8 per hidden layer, 2 fc_out_c), the same for every pass.
// What is not the MLP -- the LDS prologue, volume rendering, sky compositing, the launch helpers -- is field_composite.h, shared with
// field.hip (the (sigma, c) row store is mlp_layers.h's); the layer code (hidden_layer, out_layer and the chunk primitives under them) is mlp_f32.h,
// shared with sky_f32.hip and cnn_f32.hip; the kernel owns its LDS layout, its pass loop and the ray index it derives again for the
// epilogue.
#include <type_traits>

#include "field_composite.h"
#include "mlp_f32.h"

namespace {

constexpr int N_CHUNKS = 4 + 5 * 8 + 2;     // fc_1 | fc_2 .. fc_6 | fc_out_c; even, so a chunk's buffer is its index & 1
constexpr size_t PACKED_F32_FLOATS = (size_t)N_CHUNKS * CHUNK_FLOATS;
static_assert(PACKED_F32_FLOATS == (size_t)HID * FEAT + 5 * HID * HID + OUTC * HID, "the stream holds every weight once");

constexpr int F32_LDS_CONST = 0;                                          // fp32 constant block (the layout of mlp_layers.h)
constexpr int F32_LDS_SCALES = F32_LDS_CONST + ((C_TOTAL * 4 + 255) / 256) * 256;
constexpr int F32_LDS_LIN = F32_LDS_SCALES + NLEV * 4;
constexpr int F32_LDS_LUT = F32_LDS_LIN + MAX_LIN * 4;
constexpr int F32_LDS_TOTAL = F32_LDS_LUT + 1024;

constexpr int F32_FIELD = 0, F32_RAW = 1, F32_FIELD_AUX = 2;

struct F32Params {
    const float *wpk;          // packed f32 weights (pack_f32_kernel)
    const float *consts;       // fp32 constant block, fc_sigma's weights UNSCALED
    const float *sky_c;        // [n_src, 64]
    const float *sky_avg;      // dev [64]
    float *net_out;            // FIELD: [R, 64]; RAW: c [R, 64]
    int32_t R, ns, nch, n_tiles;
    RayWindow win;
    EncParams enc;
    const float *cam_ori_dev;  // optional dev f32 [3] (overrides enc.ori)
    const float *x;            // RAW: [R, 128]
    const uint8_t *label;      // RAW: [R]
    float *sigma_out;          // RAW: [R]
    // FIELD_AUX: the other return values of Generator._forward_perpix, each optional (field.hip MlpParams has the same six)
    float *w_out;              // [R][ns]     weights, * !sky_only (scenedreamer.py:373-376)
    float *depth_out;          // [R][ns]     rand_depth after the NaN / inf -> 0 replacement (:350-352)
    float *sig_out;            // [R][ns]     net_out_s (layers.py:115)
    float *col_out;            // [R][ns][64] net_out_c (layers.py:125)
    float *skyb_out;           // [R][64]     skynet_out_c after the keep_sky_out blend (:401)
    uint8_t *nosky_out;        // [R]         nosky_mask (:382-383)
};

template <int MODE>
__global__ __launch_bounds__(256, 1) void field_f32_kernel(const F32Params p) {
    constexpr bool RAW = MODE == F32_RAW, AUX = MODE == F32_FIELD_AUX;
    // The two weight buffers are two OBJECTS on purpose: hipcc's wait insertion then knows that the LDS-DMA into one cannot
    // alias the fragment reads from the other and waits for the DMA (vmcnt) only at the __syncthreads() that ends the chunk.
    // As halves of one array every first fragment read of a chunk waited for the prefetch issued just before it.
    __shared__ __attribute__((aligned(1024))) char wb0[CHUNK_BYTES];
    __shared__ __attribute__((aligned(1024))) char wb1[CHUNK_BYTES];
    __shared__ __attribute__((aligned(1024))) char lds[F32_LDS_TOTAL];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31, q = j & 3;
    const unsigned lane16 = lane * 16;
    const WeightBuffers ws{p.wpk, wb0, wb1, wave, lane, lane16};

    chunk_fetch(p.wpk, wb0, 0, wave, lane16);
    float *cst = reinterpret_cast<float *>(lds + F32_LDS_CONST);
    stage_consts(cst, p.consts, p.sky_avg);
    EncParams enc = p.enc;
    if constexpr (!RAW)   // the encode stage reads its small tables from LDS, as in field_kernel
        stage_enc_tables(enc, p.enc, reinterpret_cast<float *>(lds + F32_LDS_SCALES), reinterpret_cast<float *>(lds + F32_LDS_LIN),
                         reinterpret_cast<uint8_t *>(lds + F32_LDS_LUT), p.cam_ori_dev);
    __syncthreads();   // chunk 0 and the tables are in place.  From here on: at a pass's start chunk 0 sits in buffer 0

    const int n_groups = (p.n_tiles + 3) >> 2;
    for (int grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const int tile = grp * 4 + wave;
        const bool tile_ok = tile < p.n_tiles;
        const int ray = tile * RAYS_PER_TILE + (j >> 2);
        const bool ray_ok = !RAW && tile_ok && ray < p.R && p.win.valid(ray);
        const int rl = ray_ok ? ray : p.R - 1;
        const int rr = RAW ? 0 : enc.win.src(rl);
        uint8_t flag = 0;                                  // bit 0 sky_only, bit 1 nosky
        if constexpr (!RAW) flag = (ray_ok && enc.voxel_id[(size_t)rr * enc.M] != 0) ? (uint8_t)0 : (uint8_t)1;   // scenedreamer.py:337
        // a group none of whose 32 rays hits anything is skipped: every weight is exactly zero (:376)
        // (AUX also returns the per-sample sigma / colour of rays that hit nothing, so it skips no group)
        const bool grp_hit = (RAW || AUX) ? true : __syncthreads_or(!(flag & 1)) != 0;
        bool gnd = false;
        float outq[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        float carry = 0.f, tsum = 0.f;

        for (int ch = 0; grp_hit && ch < p.nch; ch++) {
            int lab;
            float dist = 0.f;
            float smp_depth = 0.f;   // AUX: this lane's sample depth
            float feat[8][8];
            const long row = (long)(tile_ok ? tile : 0) * 256 + ch * 32 + j;   // RAW: this lane's row
            if constexpr (RAW) {
                const long rc = row < p.R ? row : (long)p.R - 1;               // (lanes past the end evaluate the last row, store nothing)
                lab = p.label[rc];
                const float *src = p.x + rc * FEAT + 8 * h;                    // k-step (s, c), lane half h = feature 16 s + 8 h + c
#pragma unroll
                for (int s = 0; s < 8; s++) {
                    const float4 a = *reinterpret_cast<const float4 *>(src + 16 * s), b = *reinterpret_cast<const float4 *>(src + 16 * s + 4);
                    feat[s][0] = a.x; feat[s][1] = a.y; feat[s][2] = a.z; feat[s][3] = a.w;
                    feat[s][4] = b.x; feat[s][5] = b.y; feat[s][6] = b.z; feat[s][7] = b.w;
                }
            } else {
                RayBoxes rb;
                float dd[3];
                enc_load_ray(enc, rr, rb, dd);
                const EncSample es = enc_place(enc, rb, dd, rl, ch * SAMP_PER_STEP + (j & 3), ray_ok);
                gnd = gnd || es.gnd;
                lab = es.label;
                dist = es.dist;
                if constexpr (AUX) smp_depth = es.depth;
                const bool use_feat = AUX ? ray_ok : !(flag & 1);
                // Gathers in flight per lane: 2 levels (32 x 16 B), then one at a time (field_kernel: 4 levels).  The features stay
                // f32 here -- 64 registers per lane by the end of the stage -- and a pass is 377 k matrix cycles long: a few more round
                // trips to L2 cost little, spilling would cost more
                auto gather = [&](auto nb, int s0) {
                    constexpr int NB = decltype(nb)::value;
                    float res[NB][8];
                    enc_levels<NB>(enc, es, s0, h, use_feat, res);
#pragma unroll
                    for (int t = 0; t < NB; t++)
#pragma unroll
                        for (int c = 0; c < 8; c++) feat[s0 + t][c] = res[t][c];
                };
                gather(std::integral_constant<int, 2>{}, 0);
                gather(std::integral_constant<int, 2>{}, 2);
#pragma unroll
                for (int s = 4; s < 8; s++) gather(std::integral_constant<int, 1>{}, s);
            }
            lab = lab < NLAB ? lab : NLAB - 1;   // (the table has 12 rows; a label outside it must not read past the block)

            f32x16 acc[8];
#pragma unroll
            for (int ib = 0; ib < 8; ib++) acc[ib] = zero16();
            float act[8][16];
            // ---- fc_1: chunks 0..3, chunk c = levels pairs s = 2 c, 2 c + 1 x 8 channels -------------------------------------
#pragma unroll
            for (int c = 0; c < 4; c++) {
                chunk_fetch(p.wpk, (c & 1) ? wb0 : wb1, c + 1, wave, lane16);
                float b[16];
#pragma unroll
                for (int kk = 0; kk < 16; kk++) b[kk] = feat[2 * c + (kk >> 3)][kk & 7];
                chunk_mul8((c & 1) ? wb1 : wb0, lane, b, acc);
                __syncthreads();
            }
            activate(acc, cst + C_LABEL_BIAS + lab * HID, h, act);     // fc_1(x) + fc_m_a(m), layers.py:105-109
            // ---- fc_2 .. fc_6: chunks 4 + 8 l + b, b = input block --------------------------------------------------------------
            float part = 0.f;
#pragma unroll 1
            for (int l = 0; l < 5; l++) {
                hidden_layer(ws, 4 + 8 * l, act, acc);
                activate(acc, cst + C_BETA + l * HID, h, act);
                if (l == 2) {   // fc_sigma on fc_4's activations (layers.py:115): this lane's 128 channels, then the other half's
                    const float *wsig = cst + C_WSIGMA;
#pragma unroll
                    for (int ib = 0; ib < 8; ib++)
#pragma unroll
                        for (int g = 0; g < 4; g++) {
                            const float4 wv = *reinterpret_cast<const float4 *>(wsig + 32 * ib + 8 * g + 4 * h);
                            part = fmaf(wv.x, act[ib][4 * g + 0], part);
                            part = fmaf(wv.y, act[ib][4 * g + 1], part);
                            part = fmaf(wv.z, act[ib][4 * g + 2], part);
                            part = fmaf(wv.w, act[ib][4 * g + 3], part);
                        }
                }
            }
            // ---- fc_out_c: chunks 44, 45, and chunk 0 of the next pass behind them ------------------------------------------------------
            f32x16 col[2];
            out_layer(ws, N_CHUNKS - 2, 0, act, cst + C_BC, h, col);
            const float sigma = part + __shfl_xor(part, 32) + cst[C_BSIGMA];
            if constexpr (RAW) {   // LightningMLP.forward's outputs for this lane's row: (sigma, c), layers.py:115, :125
                if (tile_ok && row < p.R) {
                    if (h == 0) p.sigma_out[row] = sigma;
                    store_colour_row(p.net_out + (size_t)row * OUTC, col, h);
                }
                continue;
            }
            // ---- volume rendering + this pass's share of the ray's colour (field_composite.h) ------------------------------------
            const float wgt = render_weight(sigma, dist, q, carry);
            tsum += wgt;
            if constexpr (AUX) {   // the per-sample return values of Generator._forward_perpix
                const int sidx = ch * SAMP_PER_STEP + q;
                if (ray_ok && sidx < p.ns) {
                    int ray_s = rl;   // (an opaque copy, as in the epilogue: the row is derived here, not carried through the pass)
                    asm volatile("" : "+v"(ray_s));
                    const size_t smp = (size_t)p.win.out_row(ray_s) * p.ns + sidx;
                    if (h == 0) {
                        if (p.w_out) p.w_out[smp] = (flag & 1) ? 0.f : wgt;
                        if (p.depth_out) p.depth_out[smp] = smp_depth;
                        if (p.sig_out) p.sig_out[smp] = sigma;
                    }
                    if (p.col_out) store_colour_row(p.col_out + smp * OUTC, col, h);
                }
            }
            accumulate_colour(col, wgt, q, outq);
        }

        // ---- blend the sky, store --------------------------------------------------------------------------------------------
        if constexpr (!RAW) {
            // (the ray's addresses are derived again from an opaque copy of its index: computed at the group's start they would
            //  be carried through every pass, in scratch memory)
            int ray_e = rl;
            asm volatile("" : "+v"(ray_e));
            const int rr_e = enc.win.src(ray_e);
            // nosky = the ray's last intersection is a voxel, or one of its samples lies at world x <= 1 (:335, :382)
            const int g = quad_any(gnd);
            const bool last_hit = ray_ok && enc.voxel_id[(size_t)rr_e * enc.M + (enc.M - 1)] != 0;
            if (last_hit || g) flag |= 2;
            blend_sky_store<AUX>(cst, p.sky_c, p.net_out, rr_e, p.win.out_row(ray_e), ray_ok, tsum, flag, outq, q, h,
                                 AUX ? p.skyb_out : nullptr, AUX ? p.nosky_out : nullptr);
        }
    }
    __syncthreads();   // (a pass's last fetch -- chunk 0 for a pass that never came -- lands before the LDS is released)
}

// ---- the packed stream --------------------------------------------------------------------------------------------------------
// The decodes are chunk_pos8 / chunk_pos2 / mlp_stream_weight (mlp_f32.h) spelled out: called, they cost this kernel a register (9 -> 10
// or 11 VGPRs, profiles/f32_layer_refactor.md).  tests/test_f32_pack_gpu.py holds it to the same layout as the other two pack kernels.
__global__ __launch_bounds__(256) void pack_f32_kernel(const MlpPackF32<5> p) {   // wh: W * alpha already folded
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;   // one thread per float of the stream
    if (g >= PACKED_F32_FLOATS) return;
    const int cp = (int)(g / CHUNK_FLOATS), rem = (int)(g % CHUNK_FLOATS);
    float v;
    if (cp < N_CHUNKS - 2) {
        const int kk = rem / 512, in = rem % 512, ib = 4 * (in / 256) + (in & 3), lane = (in % 256) / 4, h = lane >> 5, row = 32 * ib + (lane & 31);
        if (cp < 4) v = p.w1[(size_t)row * FEAT + 16 * (2 * cp + (kk >> 3)) + 8 * h + (kk & 7)];
        else v = p.wh[(cp - 4) / 8][(size_t)row * HID + 32 * ((cp - 4) % 8) + kmap_f32(kk, h)];
    } else {
        const int kk = rem / 128, in = rem % 128, ib = in & 1, lane = in / 2, h = lane >> 5, row = 32 * ib + (lane & 31);
        v = p.wc[(size_t)row * HID + 32 * (4 * (cp - (N_CHUNKS - 2)) + (kk >> 4)) + kmap_f32(kk & 15, h)];
    }
    p.out[g] = v;
}

}  // namespace

extern "C" {

size_t sdn_field_f32_packed_weight_bytes(void) { return PACKED_F32_FLOATS * sizeof(float); }
size_t sdn_field_f32_consts_floats(void) { return C_TOTAL; }

int sdn_field_pack_weights_f32(const float *w1, const float *const *wh5_host, const float *wc, void *packed, sdn_stream_t stream) {
    return pack_mlp_weights_f32<5>("sdn_field_pack_weights_f32", pack_f32_kernel, PACKED_F32_FLOATS, w1, wh5_host, wc, packed, stream);
}

// the two field entries: argument checks, parameter fill, launch.  `stochastic`: the entry accepts u_dev
static int render_f32(const char *who, bool stochastic, const int32_t *voxel_id, const float *depth2, const float *raydirs,
                      const uint8_t *lut1024, const float *table3, uint32_t table_rows, const float *scales_dev, const float *genc_host,
                      const float *cam_ori_host, const float *voxel_dims_host, const float *lin_dev, const float *u_dev, int32_t n_rays,
                      int32_t max_blocks, int32_t num_samples, float sample_depth, float dists_scale, const void *packed,
                      const float *consts, const float *sky_c, const float *sky_avg, float *net_out, int32_t n_workgroups,
                      const int32_t *window_host, const float *cam_ori_dev, int32_t strat_division, const sdn_field_aux *aux,
                      sdn_stream_t stream) {
    if (!(packed && consts && sky_c && net_out)) return sdn::fail(SDN_ERR_INVALID, "%s: null pointer", who);
    if (u_dev && !stochastic) return sdn::fail(SDN_ERR_UNSUPPORTED, "%s: deterministic sampling only (u_dev must be NULL)", who);
    if (aux && (aux->colour_passes || aux->flags))
        return sdn::fail(SDN_ERR_UNSUPPORTED, "%s: the fp32 kernel skips no colour branch (aux->colour_passes must be NULL, aux->flags 0)", who);
    if (u_dev && window_host && window_host[5] == 2)
        return sdn::fail(SDN_ERR_INVALID, "%s: stochastic sampling with the blocked == 2 ray order is not supported", who);
    static const float zero3[3] = {0.f, 0.f, 0.f};
    if (cam_ori_dev && !cam_ori_host) cam_ori_host = zero3;
    F32Params p{};
    if (int rc = fill_enc(p.enc, who, voxel_id, depth2, raydirs, lut1024, table3, table_rows, scales_dev, genc_host, cam_ori_host,
                          voxel_dims_host, lin_dev, u_dev, n_rays, max_blocks, num_samples, sample_depth, dists_scale, strat_division))
        return rc;
    int32_t launch_rays = n_rays;
    if (int rc = set_window(p.win, window_host, n_rays, who, &launch_rays)) return rc;
    p.enc.win = p.win;
    p.R = p.enc.R = launch_rays;     // (a ragged blocked window walks its whole block grid: the extra positions are no rays)
    p.ns = num_samples;
    p.nch = p.enc.nch;
    p.n_tiles = p.enc.n_tiles = sdn::div_up(launch_rays, RAYS_PER_TILE);
    p.wpk = (const float *)packed; p.consts = consts; p.sky_c = sky_c; p.sky_avg = sky_avg; p.net_out = net_out;
    p.cam_ori_dev = cam_ori_dev;
    const dim3 grid(field_workgroups(p.n_tiles, n_workgroups));
    if (aux && (aux->weights || aux->depth || aux->sigma || aux->colour || aux->sky_blended || aux->nosky)) {
        p.w_out = aux->weights; p.depth_out = aux->depth; p.sig_out = aux->sigma; p.col_out = aux->colour;
        p.skyb_out = aux->sky_blended; p.nosky_out = aux->nosky;
        hipLaunchKernelGGL((field_f32_kernel<F32_FIELD_AUX>), grid, dim3(256), 0, (hipStream_t)stream, p);
    } else {
        hipLaunchKernelGGL((field_f32_kernel<F32_FIELD>), grid, dim3(256), 0, (hipStream_t)stream, p);
    }
    return sdn::check_launch(who);
}

int sdn_field_render_f32(const int32_t *voxel_id, const float *depth2, const float *raydirs, const uint8_t *lut1024, const float *table3,
                         uint32_t table_rows, const float *scales_dev, const float *genc_host, const float *cam_ori_host,
                         const float *voxel_dims_host, const float *lin_dev, const float *u_dev, int32_t n_rays, int32_t max_blocks,
                         int32_t num_samples, float sample_depth, float dists_scale, const void *packed, const float *consts,
                         const float *sky_c, const float *sky_avg, float *net_out, int32_t n_workgroups, const int32_t *window_host,
                         const float *cam_ori_dev, sdn_stream_t stream) {
    return render_f32("sdn_field_render_f32", false, voxel_id, depth2, raydirs, lut1024, table3, table_rows, scales_dev, genc_host,
                      cam_ori_host, voxel_dims_host, lin_dev, u_dev, n_rays, max_blocks, num_samples, sample_depth, dists_scale, packed,
                      consts, sky_c, sky_avg, net_out, n_workgroups, window_host, cam_ori_dev, 0, nullptr, stream);
}

int sdn_field_render_f32_aux(const int32_t *voxel_id, const float *depth2, const float *raydirs, const uint8_t *lut1024,
                             const float *table3, uint32_t table_rows, const float *scales_dev, const float *genc_host,
                             const float *cam_ori_host, const float *voxel_dims_host, const float *lin_dev, const float *u_dev,
                             int32_t n_rays, int32_t max_blocks, int32_t num_samples, float sample_depth, float dists_scale,
                             const void *packed, const float *consts, const float *sky_c, const float *sky_avg, float *net_out,
                             int32_t n_workgroups, const int32_t *window_host, const float *cam_ori_dev, int32_t strat_division,
                             const sdn_field_aux *aux, sdn_stream_t stream) {
    return render_f32("sdn_field_render_f32_aux", true, voxel_id, depth2, raydirs, lut1024, table3, table_rows, scales_dev, genc_host,
                      cam_ori_host, voxel_dims_host, lin_dev, u_dev, n_rays, max_blocks, num_samples, sample_depth, dists_scale, packed,
                      consts, sky_c, sky_avg, net_out, n_workgroups, window_host, cam_ori_dev, strat_division, aux, stream);
}

int sdn_render_mlp_f32(const float *x, const uint8_t *label, const void *packed, const float *consts, float *sigma, float *c,
                       int64_t n_rows, int32_t n_workgroups, sdn_stream_t stream) {
    SDN_REQUIRE(x && label && packed && consts && sigma && c, "sdn_render_mlp_f32: null pointer");
    SDN_REQUIRE(n_rows > 0 && n_rows < ((int64_t)1 << 31), "sdn_render_mlp_f32: n_rows must be in [1, 2^31)");
    F32Params p{};
    p.wpk = (const float *)packed; p.consts = consts; p.net_out = c;
    p.R = (int32_t)n_rows; p.ns = 32; p.nch = 8;
    p.n_tiles = (int32_t)((n_rows + 255) / 256);
    p.win = raw_window(p.R);
    p.x = x; p.label = label; p.sigma_out = sigma;
    hipLaunchKernelGGL((field_f32_kernel<F32_RAW>), dim3(field_workgroups(p.n_tiles, n_workgroups)), dim3(256), 0, (hipStream_t)stream, p);
    return sdn::check_launch("sdn_render_mlp_f32");
}

}  // extern "C"
