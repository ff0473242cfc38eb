// The MFMA layer machinery of the register-resident MLPs, shared by the field MLP (field.hip), the sky MLP (sky.hip) and the
// render CNN's 1x1 ends (cnn_ends.hip), whose weights mlp_pack.hip packs: the packed stream layouts, the LDS weight ring, the
// activation stages and the layers built from them (layer8: 3-term f16 split, layer8x: fp6 colour layers, layer_out).  All of
// it is in an anonymous namespace, so every translation unit compiles its own force-inlined copy.  The LDS layout is the field
// kernel's; every kernel on this machinery allocates LDS_TOTAL bytes.
#pragma once

#include <utility>

#include "mfma_common.h"

namespace {

constexpr int HID = 256;        // hidden width (layers.py:62)
constexpr int FEAT = 128;       // hash-grid output width: 16 levels x 8 channels
constexpr int OUTC = 64;        // colour feature width (final_feat_dim)
constexpr int NLEV = 16;
constexpr int NLAB = 12;
constexpr int MAX_LIN = 80;     // up to 78 samples per ray
constexpr float ACT_SCALE = 0.4f; // LeakyReLU_0.2(x) = 0.4 * (1.5 x + |x|)
// The packed weights of the trunk layers fc_1 .. fc_4 carry 2^TRUNK_SHIFT (pack_kernel has the reason); the MLP kernel takes
// the factor back out of their accumulators in the activation's bias fma.  -DSDN_TRUNK_SHIFT=0 is the ablation build.
// Every layer of the sky MLP (sky_pack_kernel) and of the render CNN's chained tail (chain_pack_kernel) carries it too: their
// output layers descale in the bias fma behind layer_out (out_descale).
#ifndef SDN_TRUNK_SHIFT
#define SDN_TRUNK_SHIFT 8
#endif
constexpr int TRUNK_SHIFT = SDN_TRUNK_SHIFT;
constexpr float TRUNK_K = 1.0f / (float)(1 << TRUNK_SHIFT);

// ---- packed weight layout (in units of half8 = one lane's fragment) ---------------------------------
// layer 0: fc_1   K=128 -> 8 k-steps, 8 row blocks
// layer 1..5: fc_2..fc_6  K=256 -> 16 k-steps, 8 row blocks
// layer 6: fc_out_c  K=256 -> 16 k-steps, 2 row blocks
// fragment f of unit u of a layer sits at (u * 4 + f) * 64 + lane (unit order: see unit_coords)
constexpr size_t L0_FRAGS = 8 * 8 * 2 * 64;
constexpr size_t LH_FRAGS = 16 * 8 * 2 * 64;
constexpr size_t LO_FRAGS = 16 * 2 * 2 * 64;
constexpr size_t PACKED_FRAGS = L0_FRAGS + 5 * LH_FRAGS + LO_FRAGS;
// the input widths of the sky MLP and the render CNN's head (their kernels and their packers, mlp_pack.hip)
constexpr int SKY_IN = 33, SKY_K0 = 64;                       // sky MLP: encoded ray direction, padded to 4 k-steps
constexpr int HEAD_K = 64, HEAD_NS = HEAD_K / 16, HEAD_UNITS = HEAD_NS * 4;   // render CNN head: 16 units

// ---- fp32 constant block ----------------------------------------------------------------------------
constexpr int C_LABEL_BIAS = 0;                      // [12][256]  fc_m_a^T + fc_1.bias
constexpr int C_BETA = C_LABEL_BIAS + NLAB * HID;    // [5][256]   ModLinear output bias
constexpr int C_WSIGMA = C_BETA + 5 * HID;           // [256]
constexpr int C_BC = C_WSIGMA + HID;                 // [64]
constexpr int C_BSIGMA = C_BC + OUTC;                // [1]
constexpr int C_SKY_AVG = C_BSIGMA + 4;              // [64]
constexpr int C_TOTAL = C_SKY_AVG + OUTC;

// Exchanges inside a quad of lanes (the 4 samples of a ray in a pass) as DPP operands of the consuming VALU instruction:
// __shfl_* compiles to ds_bpermute_b32, an LDS round trip per exchange (64 of them in the volume-rendering epilogue of a pass).
template <int CTRL>
__device__ __forceinline__ float quad_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int quad_dpp(int v) {
    return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, true);
}
constexpr int QUAD_XOR1 = 0xB1;    // quad_perm [1,0,3,2]: lane ^ 1
constexpr int QUAD_XOR2 = 0x4E;    // quad_perm [2,3,0,1]: lane ^ 2
constexpr int QUAD_UP1 = 0x90;     // quad_perm [0,0,1,2]: lane - 1 (lane 0 of the quad reads itself)
constexpr int QUAD_UP2 = 0x44;     // quad_perm [0,1,0,1]: lane - 2 (lanes 0, 1 read themselves)
constexpr int QUAD_LAST = 0xFF;    // quad_perm [3,3,3,3]: the quad's last lane
constexpr int DPP_ROW_HALF_MIRROR = 0x141;   // lane i of a row of 16 reads lane i ^ 7 (reversal inside each group of 8)
constexpr int DPP_ROW_MIRROR = 0x140;        // lane i reads lane 15 - i

// f32 -> (hi, lo) f16 pair with hi + lo == x to ~2^-22 relative.  hi is rounded to NEAREST (v_cvt_pk_f16_f32, two
// values per instruction, new in gfx950): for the full 3-term product the rounding mode of hi is irrelevant (lo
// absorbs the remainder), but a layer evaluated WITHOUT the Whi.Xlo term (TERMS == 2 below) sees |x - hi| as its error:
// half as large and unbiased with round-to-nearest (tools/precision_study.py: 2.2x less output error than with
// v_cvt_pkrtz).  x - float(hi) is a single v_fma_mix_f32 reading the f16 half directly.
__device__ __forceinline__ void split8(const float (&v)[8], half8 &hi, half8 &lo) {
    unsigned int hw[4], lw[4];
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
        const half2v hp = cvt_rtn(v[e], v[e + 1]);
        const half2v lp = cvt_rtn(v[e] - (float)hp[0], v[e + 1] - (float)hp[1]);
        hw[e / 2] = __builtin_bit_cast(unsigned int, hp);
        lw[e / 2] = __builtin_bit_cast(unsigned int, lp);
    }
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    u32x4 h4 = {hw[0], hw[1], hw[2], hw[3]}, l4 = {lw[0], lw[1], lw[2], lw[3]};
    hi = __builtin_bit_cast(half8, h4);
    lo = __builtin_bit_cast(half8, l4);
}

// =====================================================================================================
// layer machinery: LDS weight ring, activation stages, layers
// =====================================================================================================
// Structure of one pass (32 samples per wave through the 7 layers):
//
//  * weights: the 4 waves of a workgroup share ONE copy of the packed weight stream (1.47 MB per pass, identical
//    for every pass).  It flows L2 -> LDS by LDS-DMA (global_load_lds, 16 B/lane, no VGPRs) into a ring of
//    4 slots x 32 KiB (= 8 units = 48 MFMAs per wave); every wave issues 8 of a slot's 32 1-KiB pieces, 3 slots
//    ahead of use, one piece behind each of the first MFMAs after the slot's barrier.
//    Per slot: counted s_waitcnt vmcnt(8) (this wave's pieces of slots g and g+1 have landed) -> raw s_barrier
//    (everybody's have, and everybody is done with slot g-1) -> DMA for slot g+3 into the position of slot g-1.
//    (8 x 16 KiB slots, 7 ahead, measured 0.9 % slower on the same box: twice the barriers.)
//    Fragments go LDS -> registers by ds_read_b128 (lane-linear image: conflict-free) through a 3-unit register
//    ring that runs across slot boundaries.  LDS read traffic 85 B/clk/CU of 256, L2 -> LDS 21 B/clk/CU.
//    (A first version fetched fragments per wave from L2: 85 B/clk/CU through a 64 B/clk/CU path, 40.8 % MFMA busy.)
//  * the kernel runs ONE wave per SIMD (the 32 samples x 256 activations as hi+lo f16 and the 32 x 256 f32
//    accumulators take 256 of the 512 registers), so a wave gets one issue slot every ~4 cycles and anything that
//    is not interleaved with MFMAs is lost matrix time (measured: MFMA-only 10.4 ms + everything-else 12.1 ms =
//    22.5 ms when the activation epilogues ran between the layers).  Therefore the layer is evaluated as
//         upper half of the outputs (row blocks 0-3) for all k, then the lower half (4-7),
//    and the bias + LeakyReLU + f16 hi/lo re-split of a finished half is executed in the shadow of the MFMAs that
//    follow it: the lower half of layer l while layer l+1 starts on k-steps 0-7 (which only need the upper half),
//    the upper half of layer l+1 during its own last k-steps 8-15 of the lower half (k-steps 0-7 of its input are
//    dead by then, so the new B fragments overwrite them).  No second accumulator set is needed.
//  * density head, volume rendering, clamp, sky blend: VALU epilogue per pass / per ray tile.
constexpr int UNITS_PER_SLOT = 8;                  // one barrier per 8 units (48 MFMAs per wave)
constexpr int NSLOT = 4;
constexpr int SLOT_BYTES = UNITS_PER_SLOT * 4096;  // 32 KiB
constexpr int DMA_AHEAD = 3;
constexpr int PIECES = SLOT_BYTES / 4096;          // 1-KiB DMA pieces per wave and slot (4 waves)
constexpr int SLOTS_PER_PASS = (8 + 5 * 16 + 4) * 4 / UNITS_PER_SLOT;   // 46
constexpr int LDS_RING = 0;
constexpr int LDS_CONST = NSLOT * SLOT_BYTES;     // fp32 constant block
constexpr int LDS_FLAGS = LDS_CONST + ((C_TOTAL * 4 + 255) / 256) * 256;
// field_kernel only: the encode stage's small tables, so that a pass's sample placement waits for no dependent global load
constexpr int LDS_ENC_SCALES = LDS_FLAGS + 64;              // f32 [16]   per-level scales
constexpr int LDS_ENC_LIN = LDS_ENC_SCALES + NLEV * 4;      // f32 [MAX_LIN] stratified positions
constexpr int LDS_ENC_LUT = LDS_ENC_LIN + MAX_LIN * 4;      // u8 [1024]  block id -> reduced label
constexpr int LDS_TIMERS = LDS_ENC_LUT + 1024;            // u32 [16]  DBG & 512: cycles per segment of a pass (timing experiments)
constexpr int LDS_TOTAL = LDS_TIMERS + 64;

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; r++) z[r] = 0.f;
    return z;
}

// a row's 64 output features -> dst[0 .. 63]: fc_out_c's accumulators (layers.py:124, gancraft_base.py:168), f16 and fp32 kernels alike
__device__ __forceinline__ void store_colour_row(float *dst, const f32x16 (&col)[2], int h) {
#pragma unroll
    for (int ib = 0; ib < 2; ib++)
#pragma unroll
        for (int g4 = 0; g4 < 4; g4++)   // registers 4 g4 .. 4 g4 + 3 of row block ib = features 32 ib + 8 g4 + 4 h + e
            *reinterpret_cast<float4 *>(dst + 32 * ib + 8 * g4 + 4 * h) =
                make_float4(col[ib][4 * g4], col[ib][4 * g4 + 1], col[ib][4 * g4 + 2], col[ib][4 * g4 + 3]);
}

struct Ring {
    int slots_per_pass;   // 92 for the field MLP, 72 for the sky MLP
    const char *wbytes;   // packed weights
    int g;                // slots consumed so far (uniform across the workgroup)
    int next_in_pass;     // slot-in-pass index of slot g + DMA_AHEAD
    int wave;             // wave index as a scalar (readfirstlane)
    int lane;
    int voff;             // per-lane byte offset of this wave's first piece inside a slot: wave*4096 + lane*16
    unsigned lds_lane;    // LDS byte address of this lane's 16 B inside fragment 0 of ring position 0
    int src_delta;        // (scalar) voff - lds_lane: what turns lds_lane into this lane's byte offset inside a slot
    int pend_global, pend_in_pass;   // slot whose refill was granted by the last ring_acquire (issued piecewise after it)
    const char *pend_src;            // this lane's source address of that refill's first piece
};

// Per-lane source address of a slot's first DMA piece = uniform slot base + this lane's offset (wave * 8 KiB + lane * 16).
// It is built HERE, per slot, by three VALU instructions inside one opaque asm block from the SGPR base and the lane's
// LDS address (a register every unit needs anyway), instead of leaving the arithmetic to hipcc: hipcc re-associates it
// into a kernel-long per-lane 64-bit base (wbytes + lane offset) plus a uniform slot offset -- two VGPRs for the whole
// kernel, which the fp6 variant spilled to scratch and reloaded at every refill behind `s_waitcnt vmcnt(0)`: a full drain
// of the DMA ring eleven times per pass in fc_5 alone (SQ_WAIT_ANY 11.5 % -> 17.6 % of the wave time).
__device__ __forceinline__ const char *ring_lane_src(const char *slot_base, const Ring &r) {
    unsigned int lo, hi;
    const unsigned int b_lo = (unsigned int)(size_t)slot_base, b_hi = (unsigned int)((size_t)slot_base >> 32);
    // lane offset = (lds_lane - lds_lane_base) + wave * PIECES * 1024, lds_lane_base + ... folded into `delta` (uniform)
    asm volatile("v_add_u32 %0, %2, %3\n\t"
                 "v_add_co_u32 %0, vcc, %4, %0\n\t"
                 "v_mov_b32 %1, %5\n\t"
                 "v_addc_co_u32 %1, vcc, 0, %1, vcc"
                 : "=&v"(lo), "=&v"(hi)
                 : "v"(r.lds_lane), "s"(r.src_delta), "s"(b_lo), "s"(b_hi)
                 : "vcc");
    return reinterpret_cast<const char *>(((size_t)hi << 32) | lo);
}

// r.lds_lane again, from nothing but the lane id.  It is the one per-lane value every unit of every layer needs (fragment reads, DMA
// source addresses), so it lives for the whole kernel -- and under the field kernel's register pressure hipcc parks it in scratch
// memory at three places; the reloads are vector-memory loads, and from then on its waitcnt pass puts `s_waitcnt vmcnt(0)` in front
// of the first use on every path a reload may have come from: right behind the hand-counted `vmcnt(8)` + barrier at the entry of
// EVERY layer (seen in the ISA of rounds 4-6: six full drains of the weight ring's DMAs per pass).  Redefining the value at each
// layer entry (three VALU instructions the compiler cannot hoist) ends the live range there: nothing to reload, nothing to wait for.
__device__ __forceinline__ void ring_refresh_lane(char *lds, Ring &r) {
    unsigned int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\t"
                 "v_mbcnt_hi_u32_b32 %0, -1, %0\n\t"
                 "v_lshl_add_u32 %0, %0, 4, %1"
                 : "=&v"(l)
                 : "s"((unsigned)(size_t)(const lds_char *)(lds + LDS_RING)));
    r.lds_lane = l;
}

template <int K>
__device__ __forceinline__ void ring_dma(const char *lane_src, char *dbase) {
    // address = this lane's source address of the slot (+ 4 KiB for the second group of four pieces) + immediate; the LDS
    // destination is wave-uniform; the instruction offset is added to the global AND to the LDS address
    // (LDS = M0 + offset + lane*16).  (The immediate is a 13-bit signed field: 4096 and up would silently wrap to
    // negative offsets.)
    __builtin_amdgcn_global_load_lds((glb_char *)(lane_src + (K / 4) * 4096), (lds_char *)(dbase + (K / 4) * 4096), 16, (K % 4) * 1024, 0);
}

__device__ __forceinline__ void ring_issue(char *lds, const Ring &r, int slot_global, int slot_in_pass) {
    const int pos = slot_global & (NSLOT - 1);
    const char *src = ring_lane_src(r.wbytes + (size_t)slot_in_pass * SLOT_BYTES, r);
    char *dbase = lds + LDS_RING + pos * SLOT_BYTES + r.wave * (PIECES * 1024);
    ring_dma<0>(src, dbase); ring_dma<1>(src, dbase); ring_dma<2>(src, dbase); ring_dma<3>(src, dbase);
    if constexpr (PIECES == 8) {
        ring_dma<4>(src, dbase); ring_dma<5>(src, dbase); ring_dma<6>(src, dbase); ring_dma<7>(src, dbase);
    }
}

// One of the 4 DMA pieces of the refill granted by the last ring_acquire.  They are issued one behind each of the next
// unit's first four MFMAs: a global_load_lds costs the issuing wave ~16 cycles of address processing, which fits in
// the shadow of a 32-cycle MFMA but was dead matrix time when all four followed the barrier back to back.
template <int K>
__device__ __forceinline__ void ring_issue_piece(char *lds, const Ring &r) {
    const int pos = r.pend_global & (NSLOT - 1);
    char *dbase = lds + LDS_RING + pos * SLOT_BYTES + r.wave * (PIECES * 1024);
    ring_dma<K>(r.pend_src, dbase);
}

// make slot r.g (and r.g+1) readable for everybody, free slot r.g-1 for its refill (ring_issue_piece<0..3>)
template <int DBG>
__device__ __forceinline__ int ring_acquire(char *lds, Ring &r) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((DMA_AHEAD - 2) * PIECES) : "memory");
    if constexpr (!(DBG & 2)) __builtin_amdgcn_s_barrier();
    r.pend_global = r.g + DMA_AHEAD;
    r.pend_in_pass = r.next_in_pass;
    r.pend_src = ring_lane_src(r.wbytes + (size_t)r.next_in_pass * SLOT_BYTES, r);
    r.next_in_pass = r.next_in_pass + 1 == r.slots_per_pass ? 0 : r.next_in_pass + 1;
    const int pos = r.g & (NSLOT - 1);
    r.g++;
    return pos;
}

// The rest of this pass's weight stream is not needed (colour branch skipped): the DMA_AHEAD slots in flight hold its next
// layer.  Refill their ring positions with the first slots of the NEXT pass, exactly the state the kernel starts in.  Every
// wave owns its quarter of a slot for both the stale and the new pieces; the wait lets the stale ones land first (they were
// issued a whole layer ago: nothing is waited for in practice).  No barrier: nobody reads the positions being refilled, and the
// position of the last consumed slot (which slower waves may still be reading) is not touched.
__device__ __forceinline__ void ring_restart(char *lds, Ring &r) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int sl = 0; sl < DMA_AHEAD; sl++) ring_issue(lds, r, r.g + sl, sl);
    r.next_in_pass = DMA_AHEAD;
}

// Per-lane view of a 256-vector in the C/D register layout: element (IB, Q, e) is feature
// 32*IB + 16*Q + (e&3) + 8*(e>>2) + 4*h.
// LDS reads of the small constant tables are issued through inline asm: hipcc's waitcnt pass cannot tell them
// from reads of the DMA ring (same __shared__ array) and would otherwise put `s_waitcnt vmcnt(0)` in front of each
// one, draining the whole 7-slot DMA pipeline six times per layer (seen in the ISA; ~25 % of the kernel time).
// Weight-fragment reads (LDS ring -> registers: lds_unit, lds_frag) have HAND-COUNTED waits (mfma_common.h; left to hipcc,
// 219 lgkmcnt(0) per pass in the ISA of the previous version).  The rule
// that makes the counts static: within a unit the 4 fragment reads (one behind each of the first 4 MFMAs) are the
// LAST LDS operations issued, so "lgkmcnt(4)" at the start of unit U means "everything issued before unit U-1's
// fragment reads has landed" = unit U's fragments (issued during unit U-2), its bias blocks and all older reads.

// 4 x 16 B at p, p+32, p+64, p+96 (bytes): the 16 accumulator-layout values of one 32-row block
__device__ __forceinline__ f32x16 lds_read_block(const float *p) {
    f32x4 v0, v1, v2, v3;
    asm volatile(
        "ds_read_b128 %0, %4\n\t"
        "ds_read_b128 %1, %4 offset:32\n\t"
        "ds_read_b128 %2, %4 offset:64\n\t"
        "ds_read_b128 %3, %4 offset:96\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3)
        : "v"(lds_addr(p))
        : "memory");
    f32x16 c;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        c[e] = v0[e]; c[4 + e] = v1[e]; c[8 + e] = v2[e]; c[12 + e] = v3[e];
    }
    return c;
}

// bias vector of row block IB in accumulator layout (it seeds the accumulator: first MFMA's C operand)
template <int IB>
__device__ __forceinline__ f32x16 bias_block(const float *bias, int h) {
    return lds_read_block(bias + 32 * IB + 4 * h);
}

// Activation of 4 accumulator values (half a B fragment), cut into 6 stages of <= 6 mutually INDEPENDENT VALU
// instructions.  With one wave per SIMD instructions issue in order: a VALU instruction behind an MFMA that waits
// for the matrix pipe waits too, and back-to-back dependent VALU instructions cost ~10 cycles each.  Putting one
// stage after each of a unit's 6 MFMAs (and fencing with sched_barrier) gives every MFMA gap ~5 independent
// instructions: the activation then costs no matrix time.  (Measured before this change: the same instructions,
// emitted as per-value dependent chains after the unit's last MFMA, took 9.2 ms of a 19.2 ms kernel.)
//   fragment T = 2*IB + Q of the next layer, HS = which 4 of its 8 elements:
//   value e is accumulator register 8*Q + 4*HS + e of row block IB = feature 32*IB + 16*Q + 8*HS + e + 4*h
// The layer bias is added HERE (one v_add per value) instead of seeding the accumulators: a seed costs 16
// v_accvgpr_write per row block plus an LDS read that has to be waited for right in front of the block's first MFMA.
// The 4 bias values (and, for fc_4, the 4 density-head weights) of a half fragment are fetched one unit ahead
// (ActIn), in front of that unit's fragment prefetches, so the unit-start wait covers them.
struct ActRegs {
    float x[4], y[4];
    half2v hp[2], lp[2];
};

struct ActIn {
    f32x4 b;   // bias of the 4 features
    f32x4 w;   // density-head weights of the 4 features (SIG only)
};

// write two packed f16 pairs into dwords 2*HS, 2*HS+1 of a fragment (whole-dword moves: 16-bit element inserts
// into a half8 are lowered through scratch memory by hipcc)
template <int HS>
__device__ __forceinline__ void put_pairs(half8 &frag, half2v p0, half2v p1) {
    u32x4v t = __builtin_bit_cast(u32x4v, frag);
    t[2 * HS] = __builtin_bit_cast(unsigned int, p0);
    t[2 * HS + 1] = __builtin_bit_cast(unsigned int, p1);
    frag = __builtin_bit_cast(half8, t);
}

// issue (no wait) the LDS reads of a half fragment's activation inputs
template <int T, int HS, bool SIG>
__device__ __forceinline__ void act_fetch(const float *bias, const float *wsig, int h, ActIn &in) {
    constexpr int F = 32 * (T / 2) + 16 * (T % 2) + 8 * HS;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(in.b) : "v"(lds_addr(bias + 4 * h)), "n"(F * 4));
    if constexpr (SIG) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(in.w) : "v"(lds_addr(wsig + 4 * h)), "n"(F * 4));
}

// LO = false: the consumer of this fragment is a 2-term layer (no Whi.Xlo product): only hi is produced
template <int T, int HS, bool SIG, int STAGE, bool LO = true>
__device__ __forceinline__ void act_stage(const f32x16 (&acc)[8], const ActIn &in, half8 (&bh)[16], half8 (&bl)[16],
                                          float &part, ActRegs &g, float k = 1.f) {
    constexpr int IB = T / 2, Q = T % 2;
    if constexpr (STAGE == 0) {
#pragma unroll
        for (int e = 0; e < 4; e++) g.y[e] = acc[IB][8 * Q + 4 * HS + e];                 // 4 x v_accvgpr_read
    } else if constexpr (STAGE == 1) {
#pragma unroll
        for (int e = 0; e < 4; e++) g.y[e] = __builtin_fmaf(g.y[e], k, in.b[e]);   // k == 1 (a literal): folds to v_add
    } else if constexpr (STAGE == 2) {
        // a' = 1.5 x + |x| = LeakyReLU_0.2(x) / 0.4 : ONE v_fma (|x| is a free source modifier); the 0.4 lives in
        // the next layer's packed weights and in the density-head weights
#pragma unroll
        for (int e = 0; e < 4; e++) g.x[e] = __builtin_fmaf(g.y[e], 1.5f, __builtin_fabsf(g.y[e]));
    } else if constexpr (STAGE == 3) {
        g.hp[0] = cvt_rtn(g.x[0], g.x[1]);
        g.hp[1] = cvt_rtn(g.x[2], g.x[3]);
        if constexpr (SIG) part += in.w[0] * g.x[0] + in.w[1] * g.x[1] + in.w[2] * g.x[2] + in.w[3] * g.x[3];
    } else if constexpr (STAGE == 4) {
        if constexpr (!LO) return;
        // remainder x - float(hi) in one v_fma_mix_f32 per value (reads the f16 half directly)
        const unsigned int p0 = __builtin_bit_cast(unsigned int, g.hp[0]), p1 = __builtin_bit_cast(unsigned int, g.hp[1]);
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(g.y[0]) : "v"(p0), "v"(g.x[0]));
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(g.y[1]) : "v"(p0), "v"(g.x[1]));
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(g.y[2]) : "v"(p1), "v"(g.x[2]));
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(g.y[3]) : "v"(p1), "v"(g.x[3]));
    } else {
        put_pairs<HS>(bh[T], g.hp[0], g.hp[1]);
        if constexpr (LO) {
            g.lp[0] = cvt_rtn(g.y[0], g.y[1]);
            g.lp[1] = cvt_rtn(g.y[2], g.y[3]);
            put_pairs<HS>(bl[T], g.lp[0], g.lp[1]);
        }
    }
}

// whole half-fragment at once (used where nothing can hide it: the tail of the first layer)
template <int T, int HS, bool SIG>
__device__ __forceinline__ void act_half(const f32x16 (&acc)[8], const float *bias, const float *wsig, int h, half8 (&bh)[16],
                                         half8 (&bl)[16], float &part, float k = 1.f) {
    ActRegs g;
    ActIn in;
    act_fetch<T, HS, SIG>(bias, wsig, h, in);
    if constexpr (SIG) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(in.b), "+v"(in.w)::"memory");
    else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(in.b)::"memory");
    act_stage<T, HS, SIG, 0>(acc, in, bh, bl, part, g);
    act_stage<T, HS, SIG, 1>(acc, in, bh, bl, part, g, k);
    act_stage<T, HS, SIG, 2>(acc, in, bh, bl, part, g);
    act_stage<T, HS, SIG, 3>(acc, in, bh, bl, part, g);
    act_stage<T, HS, SIG, 4>(acc, in, bh, bl, part, g);
    act_stage<T, HS, SIG, 5>(acc, in, bh, bl, part, g);
}

template <int T, bool SIG>
__device__ __forceinline__ void act_step(const f32x16 (&acc)[8], const float *bias, const float *wsig, int h, half8 (&bh)[16],
                                         half8 (&bl)[16], float &part, float k = 1.f) {
    act_half<T, 0, SIG>(acc, bias, wsig, h, bh, bl, part, k);
    act_half<T, 1, SIG>(acc, bias, wsig, h, bh, bl, part, k);
}

// The density head's contribution of a finished layer's LOWER half (fragments 8..15 = accumulators acc[4..7]) without producing
// the fragments: stages 0..3 of act_stage for half fragment J -- the very functions, in the very order, the next layer's pending
// work runs later, so the sum is bit-identical to the one that layer accumulates.  mlp_kernel uses it to know sigma of a pass
// BEFORE the colour layers start (colour-branch skipping).  The LDS reads of the bias / weight rows run one half fragment ahead.
template <int J>
__device__ __forceinline__ void sigma_half(const f32x16 (&acc)[8], const float *bias, const float *wsig, int h, half8 (&bh)[16],
                                           half8 (&bl)[16], ActIn (&in)[2], float &part, float k) {
    constexpr int T = 8 + J / 2, HS = J % 2;
    if constexpr (J + 1 < 16) {
        act_fetch<8 + (J + 1) / 2, (J + 1) % 2, true>(bias, wsig, h, in[(J + 1) & 1]);
        asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(in[J & 1].b), "+v"(in[J & 1].w)::"memory");
    } else {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(in[J & 1].b), "+v"(in[J & 1].w)::"memory");
    }
    ActRegs g;
    act_stage<T, HS, true, 0>(acc, in[J & 1], bh, bl, part, g);
    act_stage<T, HS, true, 1>(acc, in[J & 1], bh, bl, part, g, k);
    act_stage<T, HS, true, 2>(acc, in[J & 1], bh, bl, part, g);
    act_stage<T, HS, true, 3>(acc, in[J & 1], bh, bl, part, g);
}

template <int... Js>
__device__ __forceinline__ void sigma_lower_half(std::integer_sequence<int, Js...>, const f32x16 (&acc)[8], const float *bias,
                                                 const float *wsig, int h, half8 (&bh)[16], half8 (&bl)[16], float &part, float k) {
    ActIn in[2];
    act_fetch<8, 0, true>(bias, wsig, h, in[0]);
    (sigma_half<Js>(acc, bias, wsig, h, bh, bl, in, part, k), ...);
}

// One 8-row-block layer (NS k-steps) from the LDS ring.
//   pend:  activation of the PREVIOUS layer's lower half (row blocks 4-7 -> B fragments 8..15, bias_pend), one
//          half fragment per unit from unit 0 (HAS_PEND), hidden behind this layer's first MFMAs;
//   own:   activation of this layer's upper half into B fragments 0 .. NS/2-1 during the last NS/2 k-steps of
//          the lower half.
// On return acc[0..3] are consumed (except fragments t >= NS/2 when NS < 16), acc[4..7] hold the lower half.
// Every index below is a compile-time constant (template recursion over the unit number): register arrays must
// never be indexed dynamically or they end up in scratch memory.
constexpr int RING_DEPTH = 3;   // register ring of fragment units: 2 units (384 matrix cycles) ahead of the MFMAs

struct LayerState {
    half8 ring[RING_DEPTH][4];
    ActIn in[2];                // activation inputs of the half fragment that STARTS in unit U, fetched during unit U-1 (ActPlan::SLOT)
    ActRegs g;                  // a half fragment in flight across two units (ActPlan::PHASE 1 -> 2)
    int pos_cur, pos_nxt;
};

// one LDS read of the register ring's next unit (fragment F of unit U_IN_SLOT of ring position pos)
template <int U_IN_SLOT, int F>
__device__ __forceinline__ void lds_frag(const Ring &r, int pos, half8 &dst) {
    ds_read16<U_IN_SLOT * 4096 + F * 1024>(dst, r.lds_lane + pos * SLOT_BYTES);
}

// which activation work is hidden in unit U of a layer8
//
// What one in-order wave per SIMD can hide behind a unit's MFMAs is bounded by ISSUE time, not by the matrix pipe
// (tools/unit_cost_ubench.hip): a unit of 6 MFMAs with its 5 LDS reads hides ~18 VALU instructions; the ~36 of a whole half
// fragment make it 267 cycles instead of 201.  So a 16-k-step layer whose activation work has 60 units to go to spreads it
// (SPREAD): a half fragment takes TWO units -- stages 0..2 in one (PHASE 1), 3..5 in the next (PHASE 2), its registers kept
// in LayerState::g -- except the two that the deadlines leave one unit for (PHASE 0, all six stages as before):
//   pending (previous layer's lower half -> fragments 8..15; fragment 8+k is first needed at unit 16+2k):
//       half fragment j = 0, 1 in units 0, 1;  j >= 2 in units 2j-2, 2j-1  (j = 15: units 28, 29 < 30)
//   own (this layer's upper half -> fragments 0..7; fragment T is free from unit 34+2T on):
//       half fragment j <= 13 in units 34+2j, 35+2j (fragment T from unit 34+4T);  j = 14, 15 in units 62, 63
template <int DBG, int NS, bool HAS_PEND, bool SIG_PEND, bool SIG_OWN, int U, bool SPREAD = false>
struct ActPlan {
    static constexpr bool IN_RANGE = U >= 0 && U < NS * 4;
    static constexpr int HALF = U / (2 * NS), REM = U % (2 * NS), S = REM >> 1;
    // the previous layer's lower half (fragments 8..15, half a fragment per unit over units 0..15: fragment 8+k
    // is first needed at unit 16+2k), or this layer's upper half (fragments 0..NS/2-1) during the last NS/2 k-steps
    // of the lower half
    static constexpr bool PEND = IN_RANGE && HAS_PEND && U < (SPREAD ? 30 : 16) && !(DBG & 4);
    // own: fragment T may be overwritten once k-step T has been consumed by both row blocks of this half, i.e. from
    // k-step T+1 on.  NS == 16: fragments 0..7 during k-steps 8..15; NS < 16 (first layers): fragments 0..NS-2 during
    // k-steps 1..NS-1 (the last upper-half fragments are activated after the layer, un-hidden)
    static constexpr int S0 = NS == 16 ? 8 : 1;
    static constexpr bool OWN = IN_RANGE && (SPREAD ? U >= 34 : (HALF == 1 && S >= S0)) && !(DBG & 4);
    static constexpr int M = U - 2 * NS - 2 * S0;
    // half fragment index within its group and the part of it done in this unit
    static constexpr int J = !SPREAD ? (PEND ? U : (OWN ? M : 0))
                             : PEND ? (U < 2 ? U : 2 + (U - 2) / 2)
                             : OWN  ? (U >= 62 ? 14 + (U - 62) : (U - 34) / 2) : 0;
    static constexpr int PHASE = !SPREAD ? 0 : PEND ? (U < 2 ? 0 : 1 + (U - 2) % 2) : OWN ? (U >= 62 ? 0 : 1 + (U - 34) % 2) : 0;
    static constexpr int T = PEND ? 8 + J / 2 : (OWN ? J / 2 : 0);
    static constexpr int HS = J % 2;
    static constexpr bool SIG = PEND ? SIG_PEND : SIG_OWN;
    static constexpr bool ACT = PEND || OWN;
    static constexpr bool STARTS = ACT && PHASE != 2;       // its inputs are fetched one unit earlier ...
    static constexpr int SLOT = SPREAD ? J % 2 : U % 2;     // ... into this ActIn (consecutive half fragments alternate)
    // activation stage (0..5, or -1) behind MFMA K (0..5) of this unit; a half-rate unit uses the two gaps without
    // fragment reads and one of the others
    static constexpr int stage(int K) {
        return !ACT ? -1 : PHASE == 0 ? K : (K == 2 ? 0 : K == 4 ? 1 : K == 5 ? 2 : -4) + (PHASE == 2 ? 3 : 0);
    }
};

// The deadlines the schedules above rest on, checked at compile time for both plans of a 16-k-step layer: every half fragment
// of the pending group is finished before the unit that first multiplies with its fragment (16 + 2k for fragment 8 + k), no half
// fragment of the own group starts before its fragment's last use (k-step T of the lower half: units 32 + 2T, 33 + 2T), each is
// visited once per phase in consecutive units, fragments 0..3 are complete before unit 56 (where a layer feeding an MX layer
// converts K block 0), and consecutive half fragments alternate between the two ActIn slots.
template <bool SPREAD, int... Us>
constexpr bool act_plan_ok(std::integer_sequence<int, Us...>) {
    int first[2][16] = {}, last[2][16] = {}, visits[2][16] = {}, slot[2][16] = {};
    for (int g = 0; g < 2; g++)
        for (int k = 0; k < 16; k++) first[g][k] = last[g][k] = -1;
    bool ok = true;
    auto visit = [&](int U, bool pend, bool own, int j, int phase, int sl, bool starts) {
        if (!pend && !own) return;
        if (pend && own) ok = false;
        const int g = own ? 1 : 0;
        if (first[g][j] < 0) { first[g][j] = U; slot[g][j] = sl; if (!starts || phase == 2) ok = false; }
        else if (U != last[g][j] + 1 || phase != 2 || starts || sl != slot[g][j]) ok = false;
        last[g][j] = U;
        visits[g][j]++;
    };
    (visit(Us, ActPlan<0, 16, true, false, false, Us, SPREAD>::PEND, ActPlan<0, 16, true, false, false, Us, SPREAD>::OWN,
           ActPlan<0, 16, true, false, false, Us, SPREAD>::J, ActPlan<0, 16, true, false, false, Us, SPREAD>::PHASE,
           ActPlan<0, 16, true, false, false, Us, SPREAD>::SLOT, ActPlan<0, 16, true, false, false, Us, SPREAD>::STARTS), ...);
    for (int j = 0; j < 16; j++) {
        const int k = j / 2;
        if (visits[0][j] != (last[0][j] - first[0][j] + 1) || visits[1][j] != (last[1][j] - first[1][j] + 1)) ok = false;
        if (first[0][j] < 0 || last[0][j] >= 16 + 2 * k) ok = false;                        // pending: fragment 8 + k ready in time
        if (first[1][j] < 34 + 2 * k || last[1][j] > 63) ok = false;                        // own: fragment k free, done inside the layer
        if (k < 4 && last[1][j] >= 56) ok = false;                                          // K block 0 complete before its conversion
        if (j > 0 && (slot[0][j] == slot[0][j - 1] || slot[1][j] == slot[1][j - 1])) ok = false;
    }
    return ok && slot[1][0] != slot[0][15];
}
static_assert(act_plan_ok<false>(std::make_integer_sequence<int, 64>{}), "ActPlan: one half fragment per unit");
static_assert(act_plan_ok<true>(std::make_integer_sequence<int, 64>{}), "ActPlan<SPREAD>: half-rate schedule");

template <int DBG, int NS, bool HAS_PEND, bool SIG_PEND, bool SIG_OWN, int U, bool SPREAD = false>
__device__ __forceinline__ void layer8_fetch(const float *bias, const float *bias_pend, const float *wsig, int h, LayerState &st) {
    using P = ActPlan<DBG, NS, HAS_PEND, SIG_PEND, SIG_OWN, U, SPREAD>;
    if constexpr (P::STARTS) act_fetch<P::T, P::HS, P::SIG>(P::PEND ? bias_pend : bias, wsig, h, st.in[P::SLOT]);
}

// TERMS = 3: Whi.Xhi + Wlo.Xhi + Whi.Xlo (6 MFMAs per unit);  TERMS = 2: the Whi.Xlo products are dropped (4 MFMAs per
// unit; the colour layers fc_5 / fc_6, whose error is not amplified by the density head -- DESIGN.md).
// LO_PEND / LO_OWN: whether the fragments activated in this layer (previous layer's lower half / this layer's upper
// half) need their lo part, i.e. whether their CONSUMER is a 3-term layer.
// the layers whose activation work is spread at half rate (ActPlan): 16 k-steps, 6 MFMAs per unit, pending work
constexpr bool layer8_spread(int NS, bool HAS_PEND, int TERMS) { return NS == 16 && HAS_PEND && TERMS == 3; }

template <int DBG, int NS, bool HAS_PEND, bool SIG_PEND, bool SIG_OWN, int TERMS, bool LO_PEND, bool LO_OWN, int U>
__device__ __forceinline__ void layer8_unit(char *lds, Ring &r, LayerState &st, half8 (&bh)[16], half8 (&bl)[16],
                                            f32x16 (&acc)[8], const float *bias, const float *bias_pend, const float *wsig,
                                            int h, float &part, float k_own, float k_pend) {
    constexpr int UNITS = NS * 4, RD = RING_DEPTH, UPS = UNITS_PER_SLOT;
    constexpr bool SPREAD = layer8_spread(NS, HAS_PEND, TERMS) && !(DBG & 16);
    using P = ActPlan<DBG, NS, HAS_PEND, SIG_PEND, SIG_OWN, U, SPREAD>;
    if constexpr (U % UPS == 0 && U != 0) {
        st.pos_cur = ring_acquire<DBG>(lds, r);
        st.pos_nxt = (st.pos_cur + 1) & (NSLOT - 1);
    }
    constexpr int UN = U + RD - 1;
    constexpr bool PF = UN < UNITS && !(DBG & 8);
    const int pf_pos = (UN / UPS) == (U / UPS) ? st.pos_cur : st.pos_nxt;
    constexpr int S = P::S, IB = 4 * P::HALF + 2 * (P::REM & 1);
    constexpr int T = P::T, HS = P::HS;
    constexpr bool SIG = P::SIG;
    constexpr bool LO = P::PEND ? LO_PEND : LO_OWN;
    ActRegs g_unit;
    ActRegs &g = SPREAD ? st.g : g_unit;
    half8(&a)[4] = st.ring[U % RD];
    half8(&nx)[4] = st.ring[UN % RD];
    const ActIn &in = st.in[P::SLOT];
    // this unit's fragments (issued during unit U-2) and activation inputs (issued at the start of unit U-1) have
    // landed once only unit U-1's 4 fragment reads are outstanding
    constexpr bool PF_PREV = U == 0 || ((U - 1 + RD - 1) < UNITS && !(DBG & 8));
    lds_wait<PF_PREV ? 4 : 0>();
    layer8_fetch<DBG, NS, HAS_PEND, SIG_PEND, SIG_OWN, U + 1, SPREAD>(bias, bias_pend, wsig, h, st);
#define SDN_STAGE(K) \
    if constexpr (U % UPS < PIECES / 4 && K < 4 && !(DBG & 1)) ring_issue_piece<4 * (U % UPS) + ((K) & 3)>(lds, r); \
    if constexpr (P::stage(K) >= 0) act_stage<T, HS, SIG, P::stage(K) < 0 ? 0 : P::stage(K), LO>(acc, in, bh, bl, part, g, P::PEND ? k_pend : k_own); \
    if constexpr (PF && K < 4) lds_frag<UN % UPS, (K) & 3>(r, pf_pos, nx[(K) & 3]); \
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (DBG & 16) {
        asm volatile("" ::"v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(bh[S]), "v"(bl[S]));
        if constexpr (S == 0) { acc[IB] = zero16(); acc[IB + 1] = zero16(); }
        SDN_STAGE(0) SDN_STAGE(1) SDN_STAGE(2) SDN_STAGE(3) SDN_STAGE(4) SDN_STAGE(5)
    } else if constexpr (TERMS == 2) {
        // 4 MFMAs: the six activation stages share four gaps (stage 4 is empty and stage 5 a single move when !LO)
        if constexpr (S == 0) acc[IB] = mfma16(a[0], bh[S], zero16());
        else acc[IB] = mfma16(a[0], bh[S], acc[IB]);
        SDN_STAGE(0) SDN_STAGE(1)
        if constexpr (S == 0) acc[IB + 1] = mfma16(a[2], bh[S], zero16());
        else acc[IB + 1] = mfma16(a[2], bh[S], acc[IB + 1]);
        SDN_STAGE(2)
        acc[IB] = mfma16(a[1], bh[S], acc[IB]);
        SDN_STAGE(3)
        acc[IB + 1] = mfma16(a[3], bh[S], acc[IB + 1]);
        SDN_STAGE(4) SDN_STAGE(5)
    } else {
        if constexpr (S == 0) acc[IB] = mfma16(a[0], bh[S], zero16());
        else acc[IB] = mfma16(a[0], bh[S], acc[IB]);
        SDN_STAGE(0)
        if constexpr (S == 0) acc[IB + 1] = mfma16(a[2], bh[S], zero16());
        else acc[IB + 1] = mfma16(a[2], bh[S], acc[IB + 1]);
        SDN_STAGE(1)
        acc[IB] = mfma16(a[1], bh[S], acc[IB]);
        SDN_STAGE(2)
        acc[IB + 1] = mfma16(a[3], bh[S], acc[IB + 1]);
        SDN_STAGE(3)
        acc[IB] = mfma16(a[0], bl[S], acc[IB]);
        SDN_STAGE(4)
        acc[IB + 1] = mfma16(a[2], bl[S], acc[IB + 1]);
        SDN_STAGE(5)
    }
#undef SDN_STAGE
}

template <int DBG, int NS, bool HAS_PEND, bool SIG_PEND, bool SIG_OWN, int TERMS, bool LO_PEND, bool LO_OWN, int... Us>
__device__ __forceinline__ void layer8_units(std::integer_sequence<int, Us...>, char *lds, Ring &r, LayerState &st,
                                             half8 (&bh)[16], half8 (&bl)[16], f32x16 (&acc)[8], const float *bias,
                                             const float *bias_pend, const float *wsig, int h, float &part, float k_own,
                                             float k_pend) {
    (layer8_unit<DBG, NS, HAS_PEND, SIG_PEND, SIG_OWN, TERMS, LO_PEND, LO_OWN, Us>(lds, r, st, bh, bl, acc, bias, bias_pend, wsig, h, part,
                                                                                   k_own, k_pend), ...);
}

template <int DBG, int NS, bool HAS_PEND, bool SIG_PEND, bool SIG_OWN, int TERMS = 3, bool LO_PEND = true, bool LO_OWN = true>
__device__ __forceinline__ void layer8(char *lds, Ring &r, half8 (&bh)[16], half8 (&bl)[16], f32x16 (&acc)[8],
                                       const float *bias, const float *bias_pend, const float *wsig, int h, float &part,
                                       float k_own = 1.f, float k_pend = 1.f) {
    LayerState st;
    ring_refresh_lane(lds, r);
    st.pos_cur = ring_acquire<DBG>(lds, r);
    st.pos_nxt = (st.pos_cur + 1) & (NSLOT - 1);
    layer8_fetch<DBG, NS, HAS_PEND, SIG_PEND, SIG_OWN, 0, layer8_spread(NS, HAS_PEND, TERMS) && !(DBG & 16)>(bias, bias_pend, wsig, h, st);
    lds_unit<0>(r.lds_lane + st.pos_cur * SLOT_BYTES, st.ring[0]);
    lds_unit<1>(r.lds_lane + st.pos_cur * SLOT_BYTES, st.ring[1]);
    layer8_units<DBG, NS, HAS_PEND, SIG_PEND, SIG_OWN, TERMS, LO_PEND, LO_OWN>(std::make_integer_sequence<int, NS * 4>{}, lds, r, st, bh,
                                                                             bl, acc, bias, bias_pend, wsig, h, part, k_own, k_pend);
}

// =====================================================================================================
// Colour layers as  Whi.Xhi (f16)  +  block-scaled fp6 corrections  [Wlo | Whi] . [X ; Xlo]
// =====================================================================================================
// The two correction terms of the 3-term split only need ~5 significant bits (their sum is 2^-11 of the product), so in
// the layers whose error nothing amplifies (fc_5, fc_6: the colour branch) they are evaluated with
// v_mfma_scale_f32_32x32x64_f8f6f4 on fp6 (e2m3) operands: K = 64 per instruction at the issue cost of one K = 16 f16
// MFMA.  192 MFMAs per layer instead of 384; measured error of the emulation (tools/precision_study.py) 4e-5 on net_out
// against 5-7e-4 for simply dropping a term.  Operand facts (pinned on the hardware by tools/mx_probe.hip): lane l holds
// row / column l & 31 and the 32 k values 32 * (l >> 5) + i as 6-bit fields, little endian, in 6 dwords; the E8M0 scale
// byte (2^(b - 127)) of the lane's 32-value block comes from byte OPSEL of a per-lane VGPR;
// v_cvt_scalef32_pk32_fp6_f16 converts 32 f16 (16 VGPRs, element p -> field p) dividing by a power-of-two scale, round to
// nearest even, saturating at 7.5.
//   B operands: K block kb = features 64 kb .. 64 kb + 63 = B fragments 4 kb .. 4 kb + 3; a lane's 32 values are its 8
//   elements of each of the 4 fragments (the cvt instruction reads the 16 VGPRs of bh[4kb .. 4kb+3] / bl[...] as they are).
//   Per-lane scale: biased exponent of the block's max |x| minus 2 (max lands in [4, 8): at most the top value saturates),
//   the lo block uses that exponent minus 11 (|x - f16(x)| <= 2^-11 of x's binade).
//   A operands: packed by pack_mx_kernel with one scale per row and 32-k block.
typedef unsigned int u32x6v __attribute__((ext_vector_type(6)));
typedef int i32x8v __attribute__((ext_vector_type(8)));
typedef _Float16 half32 __attribute__((ext_vector_type(32)));

struct MxState {
    u32x6v x6[4], xl6[4];   // fp6 images of the hi / lo f16 fragments of K block kb
    int sx[4];              // byte 0: scale of x6[kb], byte 1: scale of xl6[kb]
    float bm[4];            // running max |x| of K block kb (reset by mx_convert)
};
// (Keeping the fp6 images in the registers of the lo fragments they replace -- bl[4kb .. 4kb+3] are dead once converted --
// was tried: hipcc then fuses the reads of neighbouring fragments into 32-byte loads of the fragment array, which sends
// the array to scratch memory; with that blocked, the contiguity constraints cost more moves and spills than the 52
// extra registers of this struct.)

__device__ __forceinline__ half32 cat4(const half8 &a, const half8 &b, const half8 &c, const half8 &d) {
    const auto ab = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    const auto cd = __builtin_shufflevector(c, d, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    return __builtin_shufflevector(ab, cd, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25,
                                   26, 27, 28, 29, 30, 31);
}

template <int KB>
__device__ __forceinline__ void mx_convert(const half8 (&bh)[16], const half8 (&bl)[16], MxState &mx) {
    int e = (int)((__builtin_bit_cast(unsigned int, mx.bm[KB]) >> 23) & 255u) - 2;
    e = e < 12 ? 12 : e;                                   // e - 11 stays a normal scale; such blocks are ~0 anyway
    const float s_hi = __builtin_bit_cast(float, (unsigned int)e << 23);
    const float s_lo = __builtin_bit_cast(float, (unsigned int)(e - 11) << 23);
    mx.x6[KB] = __builtin_amdgcn_cvt_scalef32_pk32_fp6_f16(cat4(bh[4 * KB], bh[4 * KB + 1], bh[4 * KB + 2], bh[4 * KB + 3]), s_hi);
    mx.xl6[KB] = __builtin_amdgcn_cvt_scalef32_pk32_fp6_f16(cat4(bl[4 * KB], bl[4 * KB + 1], bl[4 * KB + 2], bl[4 * KB + 3]), s_lo);
    mx.sx[KB] = e | ((e - 11) << 8);
    mx.bm[KB] = 0.f;
}

// one fp6 MFMA: A = the two 16-byte ring fragments of an fp6 weight fragment (6 dwords of fields, scale word, pad),
// B = a fp6 activation block, OPB = which byte of sb is its scale
template <int OPB>
__device__ __forceinline__ f32x16 mfma_mx(const half8 &a_lo, const half8 &a_hi, const u32x6v &b, f32x16 c, int sb) {
    // every dword of a ring fragment must stay allocated until its (asynchronous, hand-waited) ds_read has landed: the
    // pad dword of a_hi is not an MFMA operand, so it is named here -- otherwise hipcc reuses that register as a
    // temporary right behind the read's issue and the data landing later overwrites it (found the hard way:
    // tools/check_lds_hazards.py reports exactly this)
    asm volatile("" ::"v"(a_hi));
    const u32x4v w0 = __builtin_bit_cast(u32x4v, a_lo), w1 = __builtin_bit_cast(u32x4v, a_hi);
    // (a_hi's two code dwords are copied behind a_lo by two v_mov in front of every fp6 MFMA: the 6-register operand cannot
    // overlap a 4-register fragment partially, whatever the vector is built from -- tried)
    const i32x8v A = {(int)w0[0], (int)w0[1], (int)w0[2], (int)w0[3], (int)w1[0], (int)w1[1], 0, 0};
    const i32x8v B = {(int)b[0], (int)b[1], (int)b[2], (int)b[3], (int)b[4], (int)b[5], 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B, c, 2, 2, 0, (int)w1[2], OPB, sb);
}

// running block max of K block KB taken from the finished f16 hi fragments (used where the activations were not produced by
// act_stage_x: the sky MLP's first layer).  |x| as 15-bit patterns order like the values; only the exponent is used.
typedef unsigned short u16x2v __attribute__((ext_vector_type(2)));
template <int KB>
__device__ __forceinline__ void mx_block_max_f16(const half8 (&bh)[16], MxState &mx) {
    u16x2v m = {0, 0};
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const u32x4v w = __builtin_bit_cast(u32x4v, bh[4 * KB + t]);
#pragma unroll
        for (int k = 0; k < 4; k++) m = __builtin_elementwise_max(m, __builtin_bit_cast(u16x2v, w[k] & 0x7fff7fffu));
    }
    const unsigned int top = m[0] > m[1] ? m[0] : m[1];
    mx.bm[KB] = __builtin_bit_cast(float, ((top >> 10) + 112u) << 23);   // 2^(exponent of the largest |x|)
}

// act_stage + running block max (the f32 activations of stage 2 are at hand in stage 3)
template <int T, int HS, bool SIG, int STAGE, bool MXT>
__device__ __forceinline__ void act_stage_x(const f32x16 (&acc)[8], const ActIn &in, half8 (&bh)[16], half8 (&bl)[16], MxState &mx,
                                            float &part, ActRegs &g, float k = 1.f) {
    act_stage<T, HS, SIG, STAGE, true>(acc, in, bh, bl, part, g, k);
    if constexpr (MXT && STAGE == 3) {
        float m = mx.bm[T / 4];
        asm("v_max3_f32 %0, %1, |%2|, |%3|" : "=v"(m) : "v"(m), "v"(g.x[0]), "v"(g.x[1]));
        asm("v_max3_f32 %0, %1, |%2|, |%3|" : "=v"(m) : "v"(m), "v"(g.x[2]), "v"(g.x[3]));
        mx.bm[T / 4] = m;
    }
}

// KIND 0: an ordinary 3-term layer whose OUTPUT feeds an MX layer (fc_4): its upper half is activated into f16 hi/lo
//         fragments 0..7 as always, K block 0 is converted at unit 56, K block 1 by the consumer's unit 0.
// KIND 1: MX layer fed by and feeding MX (fc_5).   KIND 2: MX layer whose output feeds a 3-term layer (fc_6 -> fc_out_c).
// MX unit order (pack_mx_kernel): per output half (row blocks 4*half .. +3) and K block kb, 8 units of 4 KiB:
//   0..3  f16 fragments of k-step 4 kb + t for the half's 4 row blocks                         -> 4 MFMAs
//   4, 5  fp6 Wlo fragments of row blocks (0,1) / (2,3) of the half  x  x6[kb]                  -> 2 MFMAs each
//   6, 7  fp6 Whi fragments of row blocks (0,1) / (2,3)              x  xl6[kb]                 -> 2 MFMAs each
// The activation schedule (which half fragment is activated behind which unit) is layer8's.
template <int DBG, int KIND, bool SIG_PEND, bool SIG_OWN, int U>
__device__ __forceinline__ void layer8x_unit(char *lds, Ring &r, LayerState &st, half8 (&bh)[16], half8 (&bl)[16], MxState &mx,
                                             f32x16 (&acc)[8], const float *bias, const float *bias_pend, const float *wsig,
                                             int h, float &part, float k_own, float k_pend) {
    constexpr int NS = 16, UNITS = 64, RD = RING_DEPTH, UPS = UNITS_PER_SLOT;
    constexpr bool MXL = KIND != 0;
    constexpr bool SPREAD = !MXL;   // MX units (4 or 2 MFMAs) are issue-bound wherever the activation work goes
    using P = ActPlan<DBG, NS, true, SIG_PEND, SIG_OWN, U, SPREAD>;
    if constexpr (U % UPS == 0 && U != 0) {
        st.pos_cur = ring_acquire<DBG>(lds, r);
        st.pos_nxt = (st.pos_cur + 1) & (NSLOT - 1);
    }
    constexpr int UN = U + RD - 1;
    constexpr bool PF = UN < UNITS && !(DBG & 8);
    const int pf_pos = (UN / UPS) == (U / UPS) ? st.pos_cur : st.pos_nxt;
    constexpr int T = P::T, HS = P::HS;
    constexpr bool SIG = P::SIG;
    // does the fragment activated here feed an MX layer?  PEND fragments (8..15) feed THIS layer, OWN fragments the next
    constexpr bool MXT = P::PEND ? MXL : KIND != 2;
    // K blocks completed by the previous unit: converted in this unit's first gap
    constexpr int CONV = (MXL && U == 0) ? 1 : (MXL && U == 8) ? 2 : (MXL && U == 16) ? 3 : (KIND != 2 && U == 56) ? 0 : -1;
    ActRegs g_unit;
    ActRegs &g = SPREAD ? st.g : g_unit;
    half8(&a)[4] = st.ring[U % RD];
    half8(&nx)[4] = st.ring[UN % RD];
    const ActIn &in = st.in[P::SLOT];
    constexpr bool PF_PREV = U == 0 || ((U - 1 + RD - 1) < UNITS && !(DBG & 8));
    lds_wait<PF_PREV ? 4 : 0>();
    layer8_fetch<DBG, NS, true, SIG_PEND, SIG_OWN, U + 1, SPREAD>(bias, bias_pend, wsig, h, st);
#define SDN_STAGE(K) \
    if constexpr (U % UPS < PIECES / 4 && K < 4 && !(DBG & 1)) ring_issue_piece<4 * (U % UPS) + ((K) & 3)>(lds, r); \
    if constexpr (CONV >= 0 && K == 0) mx_convert<CONV < 0 ? 0 : CONV>(bh, bl, mx); \
    if constexpr (P::stage(K) >= 0) act_stage_x<T, HS, SIG, P::stage(K) < 0 ? 0 : P::stage(K), MXT>(acc, in, bh, bl, mx, part, g, P::PEND ? k_pend : k_own); \
    if constexpr (PF && K < 4) lds_frag<UN % UPS, (K) & 3>(r, pf_pos, nx[(K) & 3]); \
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!MXL) {
        constexpr int S = P::S, IB = 4 * P::HALF + 2 * (P::REM & 1);
        if constexpr (S == 0) acc[IB] = mfma16(a[0], bh[S], zero16());
        else acc[IB] = mfma16(a[0], bh[S], acc[IB]);
        SDN_STAGE(0)
        if constexpr (S == 0) acc[IB + 1] = mfma16(a[2], bh[S], zero16());
        else acc[IB + 1] = mfma16(a[2], bh[S], acc[IB + 1]);
        SDN_STAGE(1)
        acc[IB] = mfma16(a[1], bh[S], acc[IB]);
        SDN_STAGE(2)
        acc[IB + 1] = mfma16(a[3], bh[S], acc[IB + 1]);
        SDN_STAGE(3)
        acc[IB] = mfma16(a[0], bl[S], acc[IB]);
        SDN_STAGE(4)
        acc[IB + 1] = mfma16(a[2], bl[S], acc[IB + 1]);
        SDN_STAGE(5)
    } else {
        constexpr int HALF = U / 32, KB = (U % 32) / 8, SUB = U % 8, IB0 = 4 * HALF;
        if constexpr (SUB < 4) {
            constexpr int S = 4 * KB + SUB;
            if constexpr (S == 0) acc[IB0] = mfma16(a[0], bh[S], zero16());
            else acc[IB0] = mfma16(a[0], bh[S], acc[IB0]);
            SDN_STAGE(0) SDN_STAGE(1)
            if constexpr (S == 0) acc[IB0 + 1] = mfma16(a[1], bh[S], zero16());
            else acc[IB0 + 1] = mfma16(a[1], bh[S], acc[IB0 + 1]);
            SDN_STAGE(2)
            if constexpr (S == 0) acc[IB0 + 2] = mfma16(a[2], bh[S], zero16());
            else acc[IB0 + 2] = mfma16(a[2], bh[S], acc[IB0 + 2]);
            SDN_STAGE(3)
            if constexpr (S == 0) acc[IB0 + 3] = mfma16(a[3], bh[S], zero16());
            else acc[IB0 + 3] = mfma16(a[3], bh[S], acc[IB0 + 3]);
            SDN_STAGE(4) SDN_STAGE(5)
        } else {
            constexpr int TERM = (SUB - 4) / 2, IBA = IB0 + 2 * ((SUB - 4) % 2);
            constexpr bool ON = !(DBG & (TERM == 0 ? 32 : 64));   // ablation: DBG & 32 drops Wlo.X, DBG & 64 drops Whi.Xlo
            if constexpr (!ON) asm volatile("" ::"v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]));
            if constexpr (ON && TERM == 0) acc[IBA] = mfma_mx<0>(a[0], a[1], mx.x6[KB], acc[IBA], mx.sx[KB]);
            if constexpr (ON && TERM == 1) acc[IBA] = mfma_mx<1>(a[0], a[1], mx.xl6[KB], acc[IBA], mx.sx[KB]);
            SDN_STAGE(0) SDN_STAGE(1) SDN_STAGE(2)
            if constexpr (ON && TERM == 0) acc[IBA + 1] = mfma_mx<0>(a[2], a[3], mx.x6[KB], acc[IBA + 1], mx.sx[KB]);
            if constexpr (ON && TERM == 1) acc[IBA + 1] = mfma_mx<1>(a[2], a[3], mx.xl6[KB], acc[IBA + 1], mx.sx[KB]);
            SDN_STAGE(3) SDN_STAGE(4) SDN_STAGE(5)
        }
    }
#undef SDN_STAGE
}

template <int DBG, int KIND, bool SIG_PEND, bool SIG_OWN, int... Us>
__device__ __forceinline__ void layer8x_units(std::integer_sequence<int, Us...>, char *lds, Ring &r, LayerState &st, half8 (&bh)[16],
                                              half8 (&bl)[16], MxState &mx, f32x16 (&acc)[8], const float *bias,
                                              const float *bias_pend, const float *wsig, int h, float &part, float k_own,
                                              float k_pend) {
    (layer8x_unit<DBG, KIND, SIG_PEND, SIG_OWN, Us>(lds, r, st, bh, bl, mx, acc, bias, bias_pend, wsig, h, part, k_own, k_pend), ...);
}

template <int DBG, int KIND, bool SIG_PEND, bool SIG_OWN>
__device__ __forceinline__ void layer8x(char *lds, Ring &r, half8 (&bh)[16], half8 (&bl)[16], MxState &mx, f32x16 (&acc)[8],
                                        const float *bias, const float *bias_pend, const float *wsig, int h, float &part,
                                        float k_own = 1.f, float k_pend = 1.f) {
    LayerState st;
    ring_refresh_lane(lds, r);
    st.pos_cur = ring_acquire<DBG>(lds, r);
    st.pos_nxt = (st.pos_cur + 1) & (NSLOT - 1);
    layer8_fetch<DBG, 16, true, SIG_PEND, SIG_OWN, 0, KIND == 0>(bias, bias_pend, wsig, h, st);
    lds_unit<0>(r.lds_lane + st.pos_cur * SLOT_BYTES, st.ring[0]);
    lds_unit<1>(r.lds_lane + st.pos_cur * SLOT_BYTES, st.ring[1]);
    layer8x_units<DBG, KIND, SIG_PEND, SIG_OWN>(std::make_integer_sequence<int, 64>{}, lds, r, st, bh, bl, mx, acc, bias, bias_pend,
                                                wsig, h, part, k_own, k_pend);
}

// Output layer (2 row blocks, 16 k-steps, one unit per k-step); the lower half of the last hidden layer is
// activated behind its first 15 k-steps (OutPlan).
struct OutState {
    half8 ring[RING_DEPTH][4];
    ActIn in[2][2];
    int pos_cur, pos_nxt;
};

// which half fragment(s) of the last hidden layer's lower half unit U of the output layer activates: fragment 8+k is
// consumed by unit 8+k, so half fragment j (fragment 8 + j/2) has to be finished in a unit < 8 + j/2.  Unit 0 takes
// half fragments 0 and 1, unit u = 1..14 takes half fragment u+1 (deadline 8 + (u+1)/2 > u), unit 15 none: the
// activation VALU work is spread over 15 units instead of packed two-deep into the first 8.
template <int DBG, int U>
struct OutPlan {
    static constexpr bool ACT = U >= 0 && U < 15 && !(DBG & 4);
    static constexpr bool TWO = ACT && U == 0;
    static constexpr int J = U == 0 ? 0 : U + 1;
    static constexpr int T = ACT ? 8 + J / 2 : 8, HS = ACT ? J % 2 : 0;
};

template <int... Us>
constexpr bool out_plan_ok(std::integer_sequence<int, Us...>) {
    int done[16] = {};   // unit in which half fragment j is activated (+1), 0 = never
    bool ok = true;
    auto visit = [&](int U, bool act, bool two, int j) {
        if (!act) return;
        if (done[j]) ok = false;
        done[j] = U + 1;
        if (two) { if (done[j + 1]) ok = false; done[j + 1] = U + 1; }
    };
    (visit(Us, OutPlan<0, Us>::ACT, OutPlan<0, Us>::TWO, OutPlan<0, Us>::J), ...);
    for (int j = 0; j < 16; j++)
        if (!done[j] || done[j] - 1 >= 8 + j / 2) ok = false;   // fragment 8 + j/2 is consumed by unit 8 + j/2
    return ok;
}
static_assert(out_plan_ok(std::make_integer_sequence<int, 16>{}), "OutPlan: every half fragment is ready before its k-step");

template <int DBG, int U>
__device__ __forceinline__ void out_fetch(const float *bias_pend, int h, OutState &st) {
    using P = OutPlan<DBG, U>;
    if constexpr (P::ACT) act_fetch<P::T, P::HS, false>(bias_pend, bias_pend, h, st.in[U & 1][0]);
    if constexpr (P::TWO) act_fetch<P::T, 1, false>(bias_pend, bias_pend, h, st.in[U & 1][1]);
}

template <int DBG, int U>
__device__ __forceinline__ void out_unit(char *lds, Ring &r, OutState &st, half8 (&bh)[16], half8 (&bl)[16],
                                         const f32x16 (&acc)[8], f32x16 (&col)[2], const float *bias_pend, int h, float &part,
                                         float k_pend) {
    constexpr int UNITS = 16, RD = RING_DEPTH, UPS = UNITS_PER_SLOT;
    if constexpr (U % UPS == 0 && U != 0) {
        st.pos_cur = ring_acquire<DBG>(lds, r);
        st.pos_nxt = (st.pos_cur + 1) & (NSLOT - 1);
    }
    constexpr int UN = U + RD - 1;
    constexpr bool PF = UN < UNITS && !(DBG & 8);
    const int pf_pos = (UN / UPS) == (U / UPS) ? st.pos_cur : st.pos_nxt;
    using P = OutPlan<DBG, U>;
    constexpr bool ACT = P::ACT, TWO = P::TWO;
    constexpr int T = P::T, HS = P::HS;
    ActRegs g0, g1;
    half8(&a)[4] = st.ring[U % RD];
    half8(&nx)[4] = st.ring[UN % RD];
    const ActIn &in0 = st.in[U & 1][0], &in1 = st.in[U & 1][1];
    constexpr bool PF_PREV = U == 0 || ((U - 1 + RD - 1) < UNITS && !(DBG & 8));
    lds_wait<PF_PREV ? 4 : 0>();
    out_fetch<DBG, U + 1>(bias_pend, h, st);
#define SDN_STAGE(K) \
    if constexpr (U % UPS < PIECES / 4 && K < 4 && !(DBG & 1)) ring_issue_piece<4 * (U % UPS) + ((K) & 3)>(lds, r); \
    if constexpr (ACT) act_stage<T, HS, false, K>(acc, in0, bh, bl, part, g0, k_pend); \
    if constexpr (TWO) act_stage<T, 1, false, K>(acc, in1, bh, bl, part, g1, k_pend); \
    if constexpr (PF && K < 4) lds_frag<UN % UPS, (K) & 3>(r, pf_pos, nx[(K) & 3]); \
    __builtin_amdgcn_sched_barrier(0);
    col[0] = mfma16(a[0], bh[U], col[0]);
    SDN_STAGE(0)
    col[1] = mfma16(a[2], bh[U], col[1]);
    SDN_STAGE(1)
    col[0] = mfma16(a[1], bh[U], col[0]);
    SDN_STAGE(2)
    col[1] = mfma16(a[3], bh[U], col[1]);
    SDN_STAGE(3)
    col[0] = mfma16(a[0], bl[U], col[0]);
    SDN_STAGE(4)
    col[1] = mfma16(a[2], bl[U], col[1]);
    SDN_STAGE(5)
#undef SDN_STAGE
}

template <int DBG, int... Us>
__device__ __forceinline__ void out_units(std::integer_sequence<int, Us...>, char *lds, Ring &r, OutState &st,
                                          half8 (&bh)[16], half8 (&bl)[16], const f32x16 (&acc)[8], f32x16 (&col)[2],
                                          const float *bias_pend, int h, float &part, float k_pend) {
    (out_unit<DBG, Us>(lds, r, st, bh, bl, acc, col, bias_pend, h, part, k_pend), ...);
}

// k_pend: the descale factor of the pending layer's accumulators (TRUNK_K when its packed weights carry 2^TRUNK_SHIFT)
template <int DBG>
__device__ __forceinline__ void layer_out(char *lds, Ring &r, half8 (&bh)[16], half8 (&bl)[16], const f32x16 (&acc)[8],
                                          f32x16 (&col)[2], const float *bias_pend, int h, float &part, float k_pend = 1.f) {
    OutState st;
    ring_refresh_lane(lds, r);
    st.pos_cur = ring_acquire<DBG>(lds, r);
    st.pos_nxt = (st.pos_cur + 1) & (NSLOT - 1);
    out_fetch<DBG, 0>(bias_pend, h, st);
    lds_unit<0>(r.lds_lane + st.pos_cur * SLOT_BYTES, st.ring[0]);
    lds_unit<1>(r.lds_lane + st.pos_cur * SLOT_BYTES, st.ring[1]);
    out_units<DBG>(std::make_integer_sequence<int, 16>{}, lds, r, st, bh, bl, acc, col, bias_pend, h, part, k_pend);
}

// col = bias + k * col for an output layer whose packed weights carry 1 / k and whose accumulators were seeded with zero
__device__ __forceinline__ void out_descale(f32x16 (&col)[2], const float *bias, int h, float k) {
    const f32x16 b0 = bias_block<0>(bias, h), b1 = bias_block<1>(bias, h);
#pragma unroll
    for (int e = 0; e < 16; e++) {
        col[0][e] = __builtin_fmaf(col[0][e], k, b0[e]);
        col[1][e] = __builtin_fmaf(col[1][e], k, b1[e]);
    }
}

// DBG & 512 (timing experiment, ablation builds): cycles of workgroup-thread 0 per segment of a pass, summed in LDS --
// 0 inputs (encode stage / staging), 1 fc_1, 2..6 fc_2..fc_6, 7 fc_out_c, 8 volume rendering, 9 everything between passes of
// different groups; 10 = passes; 11 = the colour-skip decision (early sigma + ballot), 12 = passes whose colour branch was skipped.  s_memtime is an SMEM operation: the compiler waits lgkmcnt(0) for it, which is only stricter
// than the hand-counted LDS waits around it (segment boundaries have no fragment reads in flight).
template <int DBG>
__device__ __forceinline__ void seg_tick(char *lds, int idx, unsigned &tprev) {
    if constexpr (DBG & 512) {
        const unsigned now = (unsigned)__builtin_readcyclecounter();
        if (threadIdx.x == 0) reinterpret_cast<unsigned *>(lds + LDS_TIMERS)[idx] += now - tprev;
        tprev = now;
    }
}

}  // namespace
