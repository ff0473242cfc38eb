// The encode stage of the field kernels as device functions: the ray window, sample placement (mc_utils.sample_depth_batched)
// and the collapsed-table gathers, plus the host-side helpers that fill their parameters.  Shared by the f16-split field
// kernels (field.hip) and the fp32 field kernel (field_f32.hip); all of it is per translation unit (anonymous namespace / static).
#pragma once
#include "mlp_layers.h"
#include "sdn_common.h"

namespace {

constexpr int RAYS_PER_TILE = 8;
constexpr int SAMP_PER_STEP = 4;
constexpr int MAXM = 8;

// The rays of a launch are a WINDOW of the ray arrays the ray marcher wrote for the whole padded frame (the field is
// evaluated on the 4-px apron the image can depend on, a band of rows, or a chunk of either): local ray r is ray
// w = ray0 + r of a window of `cols` columns whose ray (y, x) is source ray first + y * pitch + x.  No window: cols = 0,
// source ray = ray0 + r.  Reading through the window replaces four strided-slice copies per frame on the host side.
//
// Ray ORDER of a launch (tiled_bx > 0): launch-local ray r is not pixel r of the window in row-major order but pixel
//   (4 * (b / tiled_bx) + (r & 31) / 8,  8 * (b % tiled_bx) + (r & 7)),  b = r / 32:
// the 32 rays a workgroup takes through a pass together (4 waves x 8 rays) are an 8 x 4 pixel BLOCK instead of 32 consecutive
// pixels of a row.  What a group can leave out -- the colour branch of a pass whose samples all have weight zero, the passes
// behind its last ray's saturation -- it leaves out when ALL its rays agree, and rays that are neighbours in both directions
// agree more often: measured on the benchmark frames 36 -> 40 %, 34 -> 40 %, 23 -> 32 % of the passes without colour branch
// (tools/dbg_sigma_stats.py).  A wave still reads 8 consecutive rays of a row (the same coalescing), rays are independent
// (net_out is the same bits per ray, only its per-group statistics move), the per-ray OUTPUTS stay in the window's row-major
// order (out_row).  The host sets it when the launch covers a whole window of 8k columns x 4m rows -- or (sdn_field_render only,
// `rows` > 0) a whole window of ANY size: the block grid is ceil(cols / 8) x ceil(rows / 4), the launch has that many 32-ray groups,
// and the block positions outside the window are no rays (`valid`): the reference's 570 x 990 padded frame (990 = 8 * 123 + 6)
// takes the blocked order that way.
struct RayWindow {
    int32_t n_src;             // rays in the source arrays (stride of depth2's two planes)
    int32_t pitch, first, cols, ray0;
    int32_t tiled_bx;          // 0: row-major ray order; else 8 x 4 pixel blocks, this many per block row (= ceil(cols / 8))
    int32_t rows;              // tiled + ragged: rows of the window (block positions at x >= cols or y >= rows are no rays); else 0
    // window-local pixel index (row-major) of launch-local ray r; -1: a block position outside a ragged window
    __device__ __forceinline__ int pix(int r) const {
        const int w = ray0 + r;
        if (tiled_bx == 0) return w;
        const int b = w >> 5, by = b / tiled_bx, bxi = b - by * tiled_bx;
        const int y = 4 * by + ((w & 31) >> 3), x = 8 * bxi + (w & 7);
        if (rows > 0 && (x >= cols || y >= rows)) return -1;
        return y * cols + x;
    }
    __device__ __forceinline__ bool valid(int r) const { return rows == 0 || pix(r) >= 0; }
    __device__ __forceinline__ int src(int r) const {
        int q = pix(r);
        q = q < 0 ? 0 : q;     // (a position outside the window reads the window's first ray: a valid address, discarded by the caller)
        return cols > 0 ? first + (q / cols) * pitch + (q % cols) : q;
    }
    // row of launch-local ray r in the launch's per-ray outputs / inputs that are NOT read through the window (net_out, the
    // per-sample outputs, the stratified randoms u): r itself, or -- tiled, where ray0 == 0 -- the pixel's row-major index
    __device__ __forceinline__ int out_row(int r) const { return tiled_bx == 0 ? r : pix(r); }
};


struct EncParams {
    const int32_t *voxel_id;   // [R, M]
    const float *depth2;       // [2, R, M]
    const float *raydirs;      // [R, 3]
    const uint8_t *lut;        // [1024] minecraft id -> reduced label (ignore already mapped to dirt)
    const float *table3;       // [16][T][8] collapsed table
    float *feat;               // [n_tiles][nch][8 k-steps][64 lanes][8 f16 hi | 8 f16 lo]: the MLP's B fragments, split
    float *dist;               // [n_tiles][nch][32]  new_dists * dists_scale (0 for padding samples)
    uint8_t *label;            // [n_tiles][nch][32]
    uint8_t *rayflag;          // [R] bit0 sky_only, bit1 nosky
    int32_t R, M, ns, nch, n_tiles;
    uint32_t tmask;            // T - 1
    float ori[3], delim[3];
    float sample_depth, dists_scale;
    int32_t genc_oob;          // global_enc outside [0,1] after mapping: every feature is zero
    int32_t ieee_div;          // stochastic sampling: rand / nsamples as an IEEE division (CPU reference) instead of * (1/n)
    const float *lin;          // dev [ns+1]  deterministic: linspace(0,1,ns+3)[1:-1]; stochastic: linspace(0,1,ns+2)[:-1]
    const float *u;            // dev [R][ns+1] uniform randoms of the training-time stratified sampling, or nullptr
    const float *scales;       // dev [16]    per-level scale, exp2f(l*S)*H-1 evaluated on the host
    RayWindow win;             // where ray r of this launch lives in voxel_id / depth2 / raydirs
};

struct RayBoxes {
    float t[MAXM], t2[MAXM];
    int32_t id[MAXM];
};

// Everything that feeds a DISCRETE decision of the reference (box index of a sample, the is_gnd test,
// the grid cell) is evaluated with exactly the reference's fp32 operation sequence: no FMA contraction.
struct Placed {
    float depth, dist;
    int idx;
    float raw_depth;   // heads + midpoints before the NaN / inf -> 0 replacement
    int raw_idx;       // #{accu < mid} before clamping to M - 1
};

// Position of stratified point i in [0,1) (mc_utils.py:116-125): deterministic -> lin[i]; stochastic (training)
// -> rand / nsamples + linspace(0, 1, nsamples + 1)[i], `u` being the caller's torch.rand draw for this ray.
// `rand_samples / nsamples` (tensor / Python scalar) is evaluated by PyTorch as a MULTIPLICATION by the float32 reciprocal on
// a CUDA tensor (BinaryDivTrueKernel.cu: CPU-scalar fast path, a * (1 / b)) and as an IEEE division on a CPU tensor; the
// two differ by 1 ulp when nsamples is not a power of two.  n_div = +nsamples: the CUDA reference's form (strat_division
// 0 of the entry points, the default of the host wrappers); n_div = -nsamples: the CPU form (strat_division 1), which the
// goldens recorded from the reference's CPU run were produced with.
__device__ __forceinline__ float strat_pos(const float *lin, const float *u, int n_div, int i) {
#pragma clang fp contract(off)
    if (u == nullptr) return lin[i];
    const float q = n_div > 0 ? u[i] * (1.0f / (float)n_div) : u[i] / (float)(-n_div);
    return q + lin[i];
}

__device__ __forceinline__ Placed place_sample(const RayBoxes &rb, int M, const float *lin, const float *u, int n_div, int sidx,
                                               float sample_depth) {
#pragma clang fp contract(off)
    // mc_utils.py:101-107.  torch.cumsum on the CPU (what the oracle and the golden vectors were produced
    // with) accumulates float32 inputs in double and rounds every prefix back to float; it is mirrored here
    // because a 1-ulp change of a sample depth moves a fine-level feature by up to ~1e-4.
    float accu[MAXM];
    double run_d = 0.0;
    float run = 0.f;
#pragma unroll
    for (int k = 0; k < MAXM; k++) {
        if (k < M) {
            float d = rb.t2[k] - rb.t[k];
            if (d != d) d = 0.f;
            run_d += (double)d;
            run = (float)run_d;
            accu[k] = run;
        } else {
            accu[k] = 0.f;
        }
    }
    const float total = fminf(run, sample_depth);
    // :118-135 deterministic stratified points and their midpoints
    const float s0 = strat_pos(lin, u, n_div, sidx) * total, s1 = strat_pos(lin, u, n_div, sidx + 1) * total;
    const float mid = (s1 + s0) / 2.f;
    Placed o;
    o.dist = s1 - s0;
    int idx = 0;
#pragma unroll
    for (int k = 0; k < MAXM; k++)
        if (k < M && mid > accu[k]) idx++;  // :139
    // :142-145 head of the box the sample falls into: t[0] + cumulative gaps
    float head = rb.t[0];
    double cg_d = 0.0;
#pragma unroll
    for (int k = 1; k < MAXM; k++) {
        if (k < M) {
            const float g = rb.t[k] - rb.t2[k - 1];
            cg_d += (double)g;
            const float cg = (float)cg_d;
            if (k == idx) head = cg + rb.t[0];
        }
    }
    float depth = head + mid;  // :149
    o.raw_depth = depth;
    o.raw_idx = idx;
    if (depth != depth || __builtin_isinf(depth)) depth = 0.f;  // scenedreamer.py:350-352
    o.depth = depth;
    o.idx = idx < M ? idx : M - 1;
    return o;
}

__device__ __forceinline__ float mul_add_exact(float a, float b, float c) {
#pragma clang fp contract(off)
    const float p = a * b;
    return p + c;
}

__device__ __forceinline__ float normalise_coord(float wc, float delim) {
#pragma clang fp contract(off)
    // scenedreamer.py:300 then grid.py:144:  ((wc / delim * 2 - 1) + 1) / 2
    float n = wc / delim;
    n = n * 2.f;
    n = n - 1.f;
    n = n + 1.f;
    return n / 2.f;
}

// ---- the per-sample steps of the encode stage, shared by encode_kernel (features handed to mlp_kernel through HBM) and by
// ---- field_kernel = mlp_kernel<.., FUSED> (the same steps at the start of every pass: lookup + MLP in ONE kernel) ------------
// Lane (h = lane >> 5, j = lane & 31) of a wave that owns ray tile `tile` works on ray tile * 8 + (j >> 2), sample
// 4 * ch + (j & 3) of pass ch, and on the levels 2 * s + h, s = 0..7: its 8 x 8 blended values ARE B fragment s of the MLP.
__device__ __forceinline__ void enc_load_ray(const EncParams &p, int rr, RayBoxes &rb, float (&d)[3]) {
    const size_t RS = (size_t)p.win.n_src;
#pragma unroll
    for (int k = 0; k < MAXM; k++) {
        if (k < p.M) {
            rb.t[k] = p.depth2[(size_t)rr * p.M + k];
            rb.t2[k] = p.depth2[(RS + rr) * p.M + k];
            rb.id[k] = p.voxel_id[(size_t)rr * p.M + k];
        } else {
            rb.t[k] = rb.t2[k] = __builtin_nanf("");
            rb.id[k] = 0;
        }
    }
    d[0] = p.raydirs[(size_t)rr * 3]; d[1] = p.raydirs[(size_t)rr * 3 + 1]; d[2] = p.raydirs[(size_t)rr * 3 + 2];
}

struct EncSample {
    float x0, x1, x2;     // grid coordinates in [0, 1]
    bool oob, valid, gnd; // outside the grid / a real sample of a real ray / world x <= 1 (scenedreamer.py:380)
    float dist;           // new_dists * dists_scale (0 for padding samples)
    int label;            // reduced label of the box the sample falls into
    float depth;          // rand_depth after the NaN / inf -> 0 replacement (only the AUX field kernel reads it)
};

__device__ __forceinline__ EncSample enc_place(const EncParams &p, const RayBoxes &rb, const float (&d)[3], int rl, int sidx, bool ray_ok) {
    EncSample e;
    e.valid = ray_ok && sidx < p.ns;
    const Placed pl = place_sample(rb, p.M, p.lin, p.u ? p.u + (size_t)p.win.out_row(rl) * (p.ns + 1) : nullptr, p.ieee_div ? -(p.ns + 1) : p.ns + 1,
                                   e.valid ? sidx : 0, p.sample_depth);
    const float wx = mul_add_exact(d[0], pl.depth, p.ori[0]);  // scenedreamer.py:354
    const float wy = mul_add_exact(d[1], pl.depth, p.ori[1]);
    const float wz = mul_add_exact(d[2], pl.depth, p.ori[2]);
    e.gnd = e.valid && wx <= 1.0f;                           // :380
    e.x0 = normalise_coord(wx, p.delim[0]);
    e.x1 = normalise_coord(wy, p.delim[1]);
    e.x2 = normalise_coord(wz, p.delim[2]);
    e.oob = p.genc_oob || e.x0 < 0.f || e.x0 > 1.f || e.x1 < 0.f || e.x1 > 1.f || e.x2 < 0.f || e.x2 > 1.f;
    e.dist = e.valid ? pl.dist * p.dists_scale : 0.f;
    e.depth = pl.depth;
    int id = rb.id[0];
#pragma unroll
    for (int k = 1; k < MAXM; k++) {
        id = k == pl.idx ? rb.id[k] : id;
        asm("" : "+v"(id));     // a select chain, not rb.id[pl.idx]: hipcc otherwise turns it into a dynamically indexed load
    }                           // and moves the ray's boxes to scratch memory (8 stores + 1 load per sample)
    e.label = p.lut[id & 1023];
    return e;
}

// The 8 blended channels of one level = 8 corners of the collapsed 3-D table, in three steps so that a caller can put the
// gathers of SEVERAL levels in flight before it blends any of them (field_kernel: one wave per SIMD has no other wave to hide
// a level's round trip behind): where the rows are, the rows, the blend in the reference's multiply order.
struct LevelAddr {
    float f0, f1, f2;       // fractional position inside the cell
    uint32_t off[8];        // byte offset of corner c's row from table3 (corner c: bit d of c = +1 on dimension d); 32 bits: the
                            // 16 x T x 32-byte table is far below 4 GiB, and a uniform base + 32-bit lane offset is the saddr form
                            // of global_load -- half the address registers of 64-bit pointers (64 instead of 128 per 4 levels)
};

__device__ __forceinline__ void enc_level_addr(const EncParams &p, const EncSample &e, int level, bool ok, LevelAddr &a) {
    const float scale = p.scales[level];
    float f0 = mul_add_exact(e.x0, scale, 0.5f), f1 = mul_add_exact(e.x1, scale, 0.5f), f2 = mul_add_exact(e.x2, scale, 0.5f);
    const float g0 = floorf(f0), g1 = floorf(f1), g2 = floorf(f2);
    a.f0 = f0 - g0; a.f1 = f1 - g1; a.f2 = f2 - g2;
    const uint32_t a0 = (uint32_t)g0, a1 = (uint32_t)g1 * 2654435761u, a2 = (uint32_t)g2 * 805459861u;
    const uint32_t b0 = a0 + 1u, b1 = a1 + 2654435761u, b2 = a2 + 805459861u;
    const uint32_t tb = (uint32_t)level * (p.tmask + 1u);     // first row of the level
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const uint32_t hsh = ((c & 1) ? b0 : a0) ^ ((c & 2) ? b1 : a1) ^ ((c & 4) ? b2 : a2);
        a.off[c] = (tb + (ok ? (hsh & p.tmask) : 0u)) * 32u;      // (lanes without a sample read row 0 and discard it)
    }
}

__device__ __forceinline__ void enc_level_load(const EncParams &p, const LevelAddr &a, float4 (&va)[8], float4 (&vb)[8]) {
    const char *base = reinterpret_cast<const char *>(p.table3);
#pragma unroll
    for (int c = 0; c < 8; c++) {
        va[c] = *reinterpret_cast<const float4 *>(base + a.off[c]);
        vb[c] = *reinterpret_cast<const float4 *>(base + a.off[c] + 16);
    }
}

__device__ __forceinline__ void enc_level_blend(const LevelAddr &a, const float4 (&va)[8], const float4 (&vb)[8], float (&res)[8]) {
    // res[ch] = fma(w_c, row_c[ch], res[ch]) over the corners in order, two channels per v_pk_fma_f32 (the same fused
    // multiply-add per channel as the scalar form -- bit-identical -- in half the issue slots: this stage runs with one wave
    // per SIMD inside field_kernel, where every instruction is ~4 cycles of an idle matrix pipe)
    float2v r01 = {0.f, 0.f}, r23 = {0.f, 0.f}, r45 = {0.f, 0.f}, r67 = {0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 8; c++) {
        float w = 1.f;  // same multiply order as gridencoder.cu:152-160
        w *= (c & 1) ? a.f0 : 1.f - a.f0;
        w *= (c & 2) ? a.f1 : 1.f - a.f1;
        w *= (c & 4) ? a.f2 : 1.f - a.f2;
        const float2v w2 = {w, w};
        r01 = __builtin_elementwise_fma(w2, float2v{va[c].x, va[c].y}, r01);
        r23 = __builtin_elementwise_fma(w2, float2v{va[c].z, va[c].w}, r23);
        r45 = __builtin_elementwise_fma(w2, float2v{vb[c].x, vb[c].y}, r45);
        r67 = __builtin_elementwise_fma(w2, float2v{vb[c].z, vb[c].w}, r67);
    }
    res[0] = r01[0]; res[1] = r01[1]; res[2] = r23[0]; res[3] = r23[1];
    res[4] = r45[0]; res[5] = r45[1]; res[6] = r67[0]; res[7] = r67[1];
}

// one level at a time (encode_kernel: its other waves hide the round trip); no loads at all for lanes without a sample
__device__ __forceinline__ void enc_level(const EncParams &p, const EncSample &e, int level, bool use_feat, float (&res)[8]) {
#pragma unroll
    for (int c = 0; c < 8; c++) res[c] = 0.f;
    if (!e.oob && e.valid && use_feat) {
        LevelAddr a;
        float4 va[8], vb[8];
        enc_level_addr(p, e, level, true, a);
        enc_level_load(p, a, va, vb);
        enc_level_blend(a, va, vb, res);
    }
}

// field_kernel's form: NB levels 2 * (S0 + t) + h, t = 0 .. NB-1, with all their gathers issued before the first blend, and
// branch-free: lanes without a sample gather row 0 and get zeros by selection.  The arithmetic of a lane that has a sample is
// enc_level's, bit for bit.  (NB = 4: 64 x 16 B in flight per lane, 2 round trips per pass.  A 2-deep software pipeline of
// 2-level batches was tried: its register pressure made hipcc spill, and a scratch reload is a vector-memory operation -- the
// wait for it drains every gather issued before it.  The stage moves 512 KiB per CU and pass from L2: ~4 us at the L2's
// 135 GB/s per CU whatever the schedule.)
template <int NB>
__device__ __forceinline__ void enc_levels(const EncParams &p, const EncSample &e, int s0, int h, bool use_feat, float (&res)[NB][8]) {
    const bool ok = !e.oob && e.valid && use_feat;
    LevelAddr a[NB];
    float4 va[NB][8], vb[NB][8];
#pragma unroll
    for (int t = 0; t < NB; t++) enc_level_addr(p, e, 2 * (s0 + t) + h, ok, a[t]);
#pragma unroll
    for (int t = 0; t < NB; t++) enc_level_load(p, a[t], va[t], vb[t]);
#pragma unroll
    for (int t = 0; t < NB; t++) {
        enc_level_blend(a[t], va[t], vb[t], res[t]);
#pragma unroll
        for (int c = 0; c < 8; c++) res[t][c] = ok ? res[t][c] : 0.f;
    }
}

}  // namespace

// window_host: NULL, or {n_src, pitch, first, cols, ray0} (see RayWindow)
// launch_rays (sdn_field_render only): receives the rays of the launch -- n_rays, or, for a ragged blocked window
// (window_host[5] == 2), 32 x the blocks of its ceil(cols / 8) x ceil(rows / 4) grid
static int set_window(RayWindow &w, const int32_t *window_host, int32_t n_rays, const char *who, int32_t *launch_rays = nullptr) {
    w.tiled_bx = 0;
    w.rows = 0;
    if (launch_rays) *launch_rays = n_rays;
    if (window_host == nullptr) {
        w.n_src = n_rays; w.pitch = 0; w.first = 0; w.cols = 0; w.ray0 = 0;
        return 0;
    }
    w.n_src = window_host[0]; w.pitch = window_host[1]; w.first = window_host[2]; w.cols = window_host[3]; w.ray0 = window_host[4];
    if (w.n_src <= 0 || w.cols < 0 || w.ray0 < 0 || w.first < 0 || w.pitch < 0)
        return sdn::fail(SDN_ERR_INVALID, "%s: bad ray window", who);
    if (window_host[5] == 2) {   // 8 x 4 pixel blocks over a whole window of any size: positions outside it are no rays
        if (!launch_rays) return sdn::fail(SDN_ERR_UNSUPPORTED, "%s: the ragged blocked ray order exists for sdn_field_render only", who);
        if (!(w.cols > 0 && w.ray0 == 0 && n_rays % w.cols == 0))
            return sdn::fail(SDN_ERR_INVALID, "%s: the blocked ray order needs a whole window (ray0 = 0, n_rays = rows x cols)", who);
        const int rows = n_rays / w.cols;
        w.tiled_bx = (w.cols + 7) / 8;
        if (w.cols % 8 || rows % 4) {
            w.rows = rows;
            const long lr = (long)w.tiled_bx * ((rows + 3) / 4) * 32;
            if (lr >= ((long)1 << 31)) return sdn::fail(SDN_ERR_INVALID, "%s: window too large", who);
            *launch_rays = (int32_t)lr;
        }
    } else if (window_host[5]) {   // 8 x 4 pixel blocks: the launch is the whole window, whole blocks only
        if (!(w.cols > 0 && w.cols % 8 == 0 && w.ray0 == 0 && n_rays % w.cols == 0 && (n_rays / w.cols) % 4 == 0))
            return sdn::fail(SDN_ERR_INVALID, "%s: the blocked ray order needs a whole window of 8k columns x 4m rows (ray0 = 0)", who);
        w.tiled_bx = w.cols / 8;
    }
    const long last = (long)w.ray0 + n_rays - 1;
    const long src_last = w.cols > 0 ? (long)w.first + (last / w.cols) * w.pitch + (w.cols - 1) : last;
    if (src_last >= w.n_src) return sdn::fail(SDN_ERR_INVALID, "%s: ray window reaches outside the %d source rays", who, w.n_src);
    return 0;
}

// fills the encode-stage parameters (shared by sdn_field_encode and sdn_field_render); outputs / window are set by the caller
static int fill_enc(EncParams &p, const char *who, const int32_t *voxel_id, const float *depth2, const float *raydirs,
                    const uint8_t *lut1024, const float *table3, uint32_t table_rows, const float *scales_dev, const float *genc_host,
                    const float *cam_ori_host, const float *voxel_dims_host, const float *lin_dev, const float *u_dev, int32_t n_rays,
                    int32_t max_blocks, int32_t num_samples, float sample_depth, float dists_scale, int32_t strat_division) {
    if (!(voxel_id && depth2 && raydirs && lut1024 && table3 && scales_dev && genc_host && cam_ori_host && voxel_dims_host && lin_dev))
        return sdn::fail(SDN_ERR_INVALID, "%s: null pointer", who);
    if (!(strat_division == 0 || strat_division == 1))
        return sdn::fail(SDN_ERR_INVALID, "%s: strat_division must be 0 (x * (1/n)) or 1 (x / n)", who);
    if (!(n_rays > 0 && num_samples > 0)) return sdn::fail(SDN_ERR_INVALID, "%s: empty frame", who);
    if (max_blocks < 1 || max_blocks > MAXM) return sdn::fail(SDN_ERR_UNSUPPORTED, "%s: max_blocks must be 1..8", who);
    if (num_samples + 1 > MAX_LIN) return sdn::fail(SDN_ERR_UNSUPPORTED, "%s: at most 79 samples per ray", who);
    if (!(table_rows && (table_rows & (table_rows - 1)) == 0)) return sdn::fail(SDN_ERR_INVALID, "%s: table_rows must be a power of two", who);
    p.voxel_id = voxel_id; p.depth2 = depth2; p.raydirs = raydirs; p.lut = lut1024; p.table3 = table3;
    p.feat = nullptr; p.dist = nullptr; p.label = nullptr; p.rayflag = nullptr;
    p.R = n_rays; p.M = max_blocks; p.ns = num_samples;
    p.nch = sdn::div_up(num_samples, SAMP_PER_STEP);
    p.n_tiles = sdn::div_up(n_rays, RAYS_PER_TILE);
    p.tmask = table_rows - 1;
    p.genc_oob = 0;
    for (int d = 0; d < 2; d++) {
        const float x = (genc_host[d] + 1.f) / 2.f;
        if (x < 0.f || x > 1.f) p.genc_oob = 1;
    }
    for (int i = 0; i < 3; i++) { p.ori[i] = cam_ori_host[i]; p.delim[i] = voxel_dims_host[i]; }
    p.sample_depth = sample_depth; p.dists_scale = dists_scale;
    p.lin = lin_dev;
    p.u = u_dev;
    p.ieee_div = strat_division;
    p.scales = scales_dev;
    return 0;
}
