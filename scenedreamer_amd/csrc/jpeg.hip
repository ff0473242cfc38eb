// Baseline JPEG scan encoder (sequential DCT, 8 bit, three components, 4:4:4, the standard Annex K tables, restart intervals):
// the video sample of the MJPEG-MP4 writer made on the device from the uint8 [H,W,3] pixels the PNG path writes.  It replaces the
// Pillow encode of scenedreamer_amd/mp4.py (Mp4MjpegWriter.append), and through it the reference's per-frame
// `fout.append_data(rgb)` (imaginaire/generators/scenedreamer.py:560, :631).  The host adds the header and EOI (jpeg.py).
//
// The contract is the BYTES: all arithmetic is integer, tests/jpeg_ref.py restates it in numpy and the two are compared with ==.
//
//   jpeg_transform_kernel   32 MCUs per workgroup, thread = (MCU, column): RGB -> Y Cb Cr (16-bit fixed point, clamped, - 128) with
//                           the last column / row repeated on load, the 8-point pass down the column in registers, >> 10 with rounding,
//                           the pass along the row through LDS, quantisation (round half away from zero), int16 coefficients in
//                           zigzag order [MCU][component][64] stored as whole 16-byte pieces.
//   jpeg_length_kernel      one lane per block: its bit count from its coefficients and the previous MCU's DC of the same component
//                           (0 at the start of an interval).
//   jpeg_interval_kernel    one lane per interval: bits = difference of the scanned bit counts, unstuffed bytes = ceil(bits / 8).
//   jpeg_zero_kernel        zeroes the words of the unstuffed buffer that this frame uses (the total is a device word).
//   jpeg_pack_kernel        one lane per block: code words at the block's bit offset, whole 32-bit words (big-endian bit order) combined
//                           with vector atomicOr; the last block of an interval adds the 1-padding.
//   jpeg_count_kernel       one wave per 256 unstuffed bytes: the number of 0xFF bytes.
//   jpeg_stuff_kernel       one wave per 256 unstuffed bytes: byte i of interval s goes to i + (0xFF bytes before i) + 2 s, a 0xFF is
//                           followed by 0x00, the first byte of interval s >= 1 is preceded by FF D0+((s-1) mod 8); the lane with the
//                           last byte writes the total to the device word.
//   scan_*_kernel           (int_scan.h, shared with png.hip) exclusive prefix sums of uint32 arrays (tile sums, one workgroup over
//                           the tile sums, apply), used three times: bits per block, bytes per interval, 0xFF bytes per chunk.
//
// Every sum is an integer sum, every loop over tiles / blocks / chunks is a grid-stride loop: the bytes do not depend on n_workgroups.
// The bit prefix over all blocks wraps modulo 2^32; only differences inside one interval are used (<= 65 535 * 3 * 1660 bits).
//
// SIZES.  A block is at most 22 bits of DC (the chrominance code of category 11 has 11 bits, then 11 magnitude bits) and
// 63 x 26 bits of AC (16 code + 10 magnitude): <= 1660 bits <= 208 bytes unstuffed.  Stuffing at most doubles that (416 B per block,
// 1248 B per MCU) and an interval adds at most its marker and rounding: sdn_jpeg_scan_bound = 1248 * MCUs + 3 * intervals.  The
// byte count is a uint32, so frames whose bound does not fit 32 bits are rejected (about 220 Mpixel).
//
// Stores to global memory are ordinary vector stores and vector atomics.  No float arithmetic.
#include "sdn_common.h"

namespace {

#include "int_scan.h"

constexpr int MCUS_PER_WG = 32;                 // transform kernel: 32 MCUs x 8 columns
constexpr int CHUNK = 256;                      // unstuffed bytes per wave in the count / stuff kernels
constexpr unsigned BLOCK_BYTES = 208;           // unstuffed worst case of one block

// T[k][n] = rint(8192 * c_k / 2 * cos((2n + 1) k pi / 16)), evaluated once in float64
__constant__ constexpr int DCT_T[8][8] = {
    {2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},   {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
    {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784}, {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
    {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
    {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567}, {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};

// ITU-T T.81 Annex K.1, natural (row-major) order
__constant__ constexpr uint8_t QBASE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// zigzag position of natural index k * 8 + l
__constant__ constexpr uint8_t ZZ_POS[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// Annex K.3 Huffman tables as BITS (codes per length 1 .. 16) and HUFFVAL
constexpr uint8_t DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t DC_VAL[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t AC_VAL[2][162] = {
    {1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,  66,  177,
     193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,  52,  53,  54,  55,
     56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106,
     115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
     164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211,
     212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161, 177, 193,
     9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,  41,  42,  53,  54,
     55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105,
     106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
     162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
     210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};

// (code << 5) | length per symbol, codes assigned canonically from BITS / HUFFVAL; 0 for a symbol the table does not hold
struct HuffCodes {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};

constexpr HuffCodes make_huff() {
    HuffCodes h{};
    for (int t = 0; t < 2; t++) {
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; len++) {
            for (int i = 0; i < DC_BITS[t][len - 1]; i++) h.dc[t][DC_VAL[k++]] = (code++ << 5) | (uint32_t)len;
            code <<= 1;
        }
        code = 0;
        k = 0;
        for (int len = 1; len <= 16; len++) {
            for (int i = 0; i < AC_BITS[t][len - 1]; i++) h.ac[t][AC_VAL[t][k++]] = (code++ << 5) | (uint32_t)len;
            code <<= 1;
        }
    }
    return h;
}

__constant__ HuffCodes c_huff = make_huff();

// The tables of the entropy kernels in LDS: lanes index them by their own symbols
struct HuffLds {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};

__device__ inline void load_huff(HuffLds &s) {
    for (int i = threadIdx.x; i < 2 * 16; i += WG) s.dc[i >> 4][i & 15] = c_huff.dc[i >> 4][i & 15];
    for (int i = threadIdx.x; i < 2 * 256; i += WG) s.ac[i >> 8][i & 255] = c_huff.ac[i >> 8][i & 255];
    __syncthreads();
}

__device__ inline int bit_length(int v) {  // of |v|
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}

// ---- transform --------------------------------------------------------------------------------------------------------------------
struct JpegDims {
    int32_t H, W, bw, n_mcu, Ri, n_int;
};

__global__ __launch_bounds__(WG) void jpeg_transform_kernel(const uint8_t *rgb, JpegDims d, int quality, int n_groups, int16_t *coef) {
    constexpr int MS = 3 * 64 + 1;                          // ints per MCU in LDS: odd, so that the MCUs of a wave fall on different banks
    __shared__ int s_p[MCUS_PER_WG * MS];
    __shared__ __attribute__((aligned(16))) int16_t s_q[MCUS_PER_WG * 3 * 64];
    __shared__ int s_quant[2][64];
    const int t = threadIdx.x, m = t >> 3, x = t & 7;
    if (t < 128) {
        const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
        int q = ((int)QBASE[t >> 6][t & 63] * s + 50) / 100;
        s_quant[t >> 6][t & 63] = q < 1 ? 1 : (q > 255 ? 255 : q);
    }
    for (int grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        __syncthreads();                                    // s_quant written; the previous group's s_q read
        const int mcu0 = grp * MCUS_PER_WG;
        const int mcu = min(mcu0 + m, d.n_mcu - 1);         // lanes past the last MCU evaluate the last one; nothing of theirs is stored
        const int by = mcu / d.bw, bx = mcu - by * d.bw;
        const int px = min(bx * 8 + x, d.W - 1);
        int X[3][8];
#pragma unroll
        for (int y = 0; y < 8; y++) {
            const int py = min(by * 8 + y, d.H - 1);
            const uint8_t *p = rgb + ((size_t)py * d.W + px) * 3;
            const int R = p[0], G = p[1], B = p[2];
            int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
            int Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
            int Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
            X[0][y] = min(max(Y, 0), 255) - 128;
            X[1][y] = min(max(Cb, 0), 255) - 128;
            X[2][y] = min(max(Cr, 0), 255) - 128;
        }
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int k = 0; k < 8; k++) {
                int acc = 0;
#pragma unroll
                for (int y = 0; y < 8; y++) acc += DCT_T[k][y] * X[c][y];
                s_p[m * MS + c * 64 + k * 8 + x] = (acc + 512) >> 10;
            }
        __syncthreads();
        const int l = x;                                    // this thread now owns column l of the coefficients
        int Tl[8];
#pragma unroll
        for (int xx = 0; xx < 8; xx++) Tl[xx] = DCT_T[l][xx];
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int k = 0; k < 8; k++) {
                int acc = 0;
#pragma unroll
                for (int xx = 0; xx < 8; xx++) acc += s_p[m * MS + c * 64 + k * 8 + xx] * Tl[xx];
                const unsigned q = (unsigned)s_quant[c ? 1 : 0][k * 8 + l];
                const unsigned a = (unsigned)(acc < 0 ? -acc : acc);
                const int v = (int)((a + (q << 15)) / (q << 16));
                s_q[(m * 3 + c) * 64 + ZZ_POS[k * 8 + l]] = (int16_t)(acc < 0 ? -v : v);
            }
        __syncthreads();
        // 32 MCUs x 384 B are contiguous in `coef`: 768 pieces of 16 B, three per thread
        const int4 *src = reinterpret_cast<const int4 *>(s_q);
        int4 *dst = reinterpret_cast<int4 *>(coef + (size_t)mcu0 * 3 * 64);
        const int pieces = min(MCUS_PER_WG, d.n_mcu - mcu0) * 24;
        for (int i = t; i < pieces; i += WG) dst[i] = src[i];
    }
}

// ---- lengths ------------------------------------------------------------------------------------------------------------------------
// Walks one block's symbols.  emit(code_and_length_word, extra_value, extra_bits) is called per symbol in order.
template <typename Emit>
__device__ inline void walk_block(const int16_t *blk, int prev_dc, int tbl, const HuffLds &hs, Emit emit) {
    const int4 *src = reinterpret_cast<const int4 *>(blk);
    int dc = 0, run = 0;
#pragma unroll 1
    for (int piece = 0; piece < 8; piece++) {
        const int4 w = src[piece];
        const int words[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int v = (int)(int16_t)((unsigned)words[j >> 1] >> (16 * (j & 1)));
            if (piece == 0 && j == 0) {
                dc = v;
                const int diff = dc - prev_dc;
                const int cat = bit_length(diff);
                emit(hs.dc[tbl][cat & 15], (unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1u), cat);
            } else if (v == 0) {
                run++;
            } else {
                while (run >= 16) {
                    emit(hs.ac[tbl][0xF0], 0u, 0);
                    run -= 16;
                }
                const int cat = bit_length(v);
                emit(hs.ac[tbl][(run * 16 + cat) & 255], (unsigned)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u), cat);
                run = 0;
            }
        }
    }
    if (run > 0) emit(hs.ac[tbl][0x00], 0u, 0);
}

__device__ inline int prev_dc_of(const int16_t *coef, int b, int Ri) {
    const int mcu = b / 3;
    return (mcu % Ri) == 0 ? 0 : (int)coef[(size_t)(b - 3) * 64];
}

__global__ __launch_bounds__(WG) void jpeg_length_kernel(const int16_t *coef, int n_blocks, int Ri, uint32_t *bits) {
    __shared__ HuffLds hs;
    load_huff(hs);
    for (int64_t b64 = (int64_t)blockIdx.x * WG + threadIdx.x; b64 < n_blocks; b64 += (int64_t)gridDim.x * WG) {
        const int b = (int)b64;
        uint32_t total = 0;
        walk_block(coef + (size_t)b * 64, prev_dc_of(coef, b, Ri), (b % 3) ? 1 : 0, hs,
                   [&](uint32_t cl, unsigned, int extra_bits) { total += (cl & 31u) + (uint32_t)extra_bits; });
        bits[b] = total;
    }
}

// bitpre: exclusive prefix of the block bits, n_blocks + 1 entries (modulo 2^32)
__global__ __launch_bounds__(WG) void jpeg_interval_kernel(const uint32_t *bitpre, JpegDims d, uint32_t *ibytes) {
    for (int64_t s = (int64_t)blockIdx.x * WG + threadIdx.x; s < d.n_int; s += (int64_t)gridDim.x * WG) {
        const int64_t m0 = s * d.Ri, m1 = m0 + d.Ri < d.n_mcu ? m0 + d.Ri : d.n_mcu;
        const uint32_t nbits = bitpre[m1 * 3] - bitpre[m0 * 3];
        ibytes[s] = (nbits + 7u) >> 3;
    }
}

// ioff: exclusive prefix of the interval bytes, n_int + 1 entries; ioff[n_int] is the unstuffed total
__global__ __launch_bounds__(WG) void jpeg_zero_kernel(const uint32_t *ioff, int n_int, uint32_t *words, uint32_t cap_words) {
    const uint32_t n = min((ioff[n_int] >> 2) + 2u, cap_words);
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) words[i] = 0u;
}

// ---- pack ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void jpeg_pack_kernel(const int16_t *coef, const uint32_t *bitpre, const uint32_t *ioff, JpegDims d,
                                                       uint32_t *words, uint32_t cap_words) {
    __shared__ HuffLds hs;
    load_huff(hs);
    const int n_blocks = d.n_mcu * 3;
    for (int64_t b64 = (int64_t)blockIdx.x * WG + threadIdx.x; b64 < n_blocks; b64 += (int64_t)gridDim.x * WG) {
        const int b = (int)b64;
        const int mcu = b / 3, s = mcu / d.Ri;
        const int64_t m0 = (int64_t)s * d.Ri, m1 = m0 + d.Ri < d.n_mcu ? m0 + d.Ri : d.n_mcu;
        const uint64_t pos = (uint64_t)ioff[s] * 8u + (uint32_t)(bitpre[b] - bitpre[m0 * 3]);
        uint32_t w = (uint32_t)(pos >> 5);
        int fill = (int)(pos & 31u);                // bits of word w that are in `acc` or belong to earlier blocks
        uint64_t acc = 0;                           // the low `fill` bits: this block's bits pending for word w (earlier blocks' as zeros)
        auto put = [&](uint32_t value, int nbits) {  // nbits <= 27
            acc = (acc << nbits) | value;
            fill += nbits;
            if (fill >= 32) {
                fill -= 32;
                const uint32_t out = (uint32_t)(acc >> fill);
                if (w < cap_words) atomicOr(&words[w], __builtin_bswap32(out));
                w++;
                acc &= (1ull << fill) - 1ull;
            }
        };
        walk_block(coef + (size_t)b * 64, prev_dc_of(coef, b, d.Ri), (b % 3) ? 1 : 0, hs, [&](uint32_t cl, unsigned extra, int extra_bits) {
            put(((cl >> 5) << extra_bits) | extra, (int)(cl & 31u) + extra_bits);
        });
        if ((int64_t)b == m1 * 3 - 1) {             // last block of the interval: pad to a byte boundary with 1-bits
            const int pad = (int)((0u - (bitpre[m1 * 3] - bitpre[m0 * 3])) & 7u);
            put((1u << pad) - 1u, pad);
        }
        if (fill > 0 && w < cap_words) atomicOr(&words[w], __builtin_bswap32((uint32_t)(acc << (32 - fill))));
    }
}

// ---- byte stuffing and restart markers ----------------------------------------------------------------------------------------------
__device__ inline uint32_t count_ff(uint32_t word, uint32_t valid_bytes) {  // among the first valid_bytes bytes in memory order
    uint32_t c = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) c += (j < valid_bytes && ((word >> (8 * j)) & 255u) == 255u) ? 1u : 0u;
    return c;
}

__global__ __launch_bounds__(WG) void jpeg_count_kernel(const uint32_t *words, const uint32_t *ioff, int n_int, uint32_t max_chunks,
                                                        uint32_t *ffc) {
    const uint32_t total = ioff[n_int];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * (WG / 64) + (threadIdx.x >> 6), n_waves = gridDim.x * (WG / 64);
    for (uint32_t ch = wave; ch < max_chunks; ch += n_waves) {
        const uint32_t i0 = ch * CHUNK + lane * 4;
        uint32_t c = 0;
        if (i0 < total) c = count_ff(words[i0 >> 2], min(4u, total - i0));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
        if (lane == 0) ffc[ch] = c;
    }
}

__global__ __launch_bounds__(WG) void jpeg_stuff_kernel(const uint32_t *words, const uint32_t *ioff, const uint32_t *ffpre, int n_int,
                                                        uint8_t *out, uint32_t cap, uint32_t *out_bytes) {
    const uint32_t total = ioff[n_int];
    const uint32_t n_chunks = (total + CHUNK - 1) / CHUNK;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * (WG / 64) + (threadIdx.x >> 6), n_waves = gridDim.x * (WG / 64);
    for (uint32_t ch = wave; ch < n_chunks; ch += n_waves) {
        const uint32_t i0 = ch * CHUNK + lane * 4;
        const uint32_t valid = i0 < total ? min(4u, total - i0) : 0u;
        const uint32_t word = valid ? words[i0 >> 2] : 0u;
        const uint32_t c = count_ff(word, valid);
        uint32_t incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        uint32_t ff = ffpre[ch] + incl - c;         // 0xFF bytes before byte i0
        if (valid) {
            int lo = 0, hi = n_int - 1;                 // the interval of byte i0: the last s with ioff[s] <= i0
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (ioff[mid] <= i0) lo = mid; else hi = mid - 1;
            }
            int s = lo;
            for (uint32_t j = 0; j < valid; j++) {
                const uint32_t i = i0 + j;
                while (s + 1 < n_int && ioff[s + 1] <= i) s++;
                const uint32_t byte = (word >> (8 * j)) & 255u;
                const uint32_t pos = i + ff + 2u * (uint32_t)s;
                if (pos + 1u < cap) {
                    if (s > 0 && ioff[s] == i) {
                        out[pos - 2] = 0xFF;
                        out[pos - 1] = (uint8_t)(0xD0 + ((s - 1) & 7));
                    }
                    out[pos] = (uint8_t)byte;
                    if (byte == 255u) out[pos + 1] = 0;
                }
                if (byte == 255u) ff++;
                if (i == total - 1u) *out_bytes = pos + 1u + (byte == 255u ? 1u : 0u);
            }
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct Layout {  // of the workspace, every part 256-byte aligned
    JpegDims d;
    uint32_t n_blocks, max_chunks, max_tiles;
    size_t unstuffed_bytes, scan_bound;
    size_t off_coef, off_bits, off_ibytes, off_ffc, off_tiles, off_words, total;
};

// false: the frame is outside what the encoder takes (sizes, or a scan bound that does not fit the 32-bit byte count)
bool make_layout(int H, int W, int Ri, Layout &L) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || Ri < 1 || Ri > 65535) return false;
    const uint64_t bw = (uint64_t)(W + 7) / 8, bh = (uint64_t)(H + 7) / 8, n = bw * bh, n_int = (n + Ri - 1) / Ri;
    const uint64_t bound = 6ull * BLOCK_BYTES * n + 3ull * n_int;
    if (bound >= (1ull << 32)) return false;
    L.d = JpegDims{H, W, (int32_t)bw, (int32_t)n, Ri, (int32_t)n_int};
    L.n_blocks = (uint32_t)(3 * n);
    L.scan_bound = (size_t)bound;
    L.unstuffed_bytes = (size_t)(3ull * BLOCK_BYTES * n) + 16;      // whole words past the last byte
    L.max_chunks = (uint32_t)((L.unstuffed_bytes + CHUNK - 1) / CHUNK);
    const uint32_t longest = L.n_blocks > L.max_chunks ? L.n_blocks : L.max_chunks;   // n_int <= n_blocks
    L.max_tiles = (longest + 1 + SCAN_TILE - 1) / SCAN_TILE;
    size_t o = 0;
    L.off_coef = o;   o += align256((size_t)L.n_blocks * 64 * sizeof(int16_t));
    L.off_bits = o;   o += align256(((size_t)L.n_blocks + 1) * 4);
    L.off_ibytes = o; o += align256(((size_t)n_int + 1) * 4);
    L.off_ffc = o;    o += align256(((size_t)L.max_chunks + 1) * 4);
    L.off_tiles = o;  o += align256(((size_t)L.max_tiles + 1) * 4);
    L.off_words = o;  o += align256(L.unstuffed_bytes);
    L.total = o;
    return true;
}

}  // namespace

extern "C" {

size_t sdn_jpeg_scan_bound(int H, int W, int restart_mcus) {
    Layout L;
    return make_layout(H, W, restart_mcus, L) ? L.scan_bound : 0;
}

size_t sdn_jpeg_workspace_bytes(int H, int W, int restart_mcus) {
    Layout L;
    return make_layout(H, W, restart_mcus, L) ? L.total : 0;
}

int sdn_jpeg_encode_scan(const uint8_t *rgb_hwc, int H, int W, int quality, int restart_mcus, void *workspace, uint8_t *scan,
                         uint32_t *scan_bytes_dev, int n_workgroups, sdn_stream_t stream) {
    if (quality < 1 || quality > 100) return sdn::fail(SDN_ERR_UNSUPPORTED, "sdn_jpeg_encode_scan: quality must be 1 .. 100 (got %d)", quality);
    if (restart_mcus < 1 || restart_mcus > 65535)
        return sdn::fail(SDN_ERR_UNSUPPORTED, "sdn_jpeg_encode_scan: restart_mcus must be 1 .. 65535 (got %d)", restart_mcus);
    if (H < 0 || W < 0 || H > 65535 || W > 65535)
        return sdn::fail(SDN_ERR_UNSUPPORTED, "sdn_jpeg_encode_scan: H and W must be 1 .. 65535 (got %d x %d)", H, W);
    if (H == 0 || W == 0) return SDN_OK;            // empty frame: nothing to encode
    if (!rgb_hwc || !workspace || !scan || !scan_bytes_dev) return sdn::fail(SDN_ERR_UNSUPPORTED, "sdn_jpeg_encode_scan: null pointer");
    Layout L;
    if (!make_layout(H, W, restart_mcus, L))
        return sdn::fail(SDN_ERR_UNSUPPORTED, "sdn_jpeg_encode_scan: %d x %d is too large: the scan bound does not fit 32 bits", H, W);
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    int16_t *coef = reinterpret_cast<int16_t *>(ws + L.off_coef);
    uint32_t *bits = reinterpret_cast<uint32_t *>(ws + L.off_bits);
    uint32_t *ibytes = reinterpret_cast<uint32_t *>(ws + L.off_ibytes);
    uint32_t *ffc = reinterpret_cast<uint32_t *>(ws + L.off_ffc);
    uint32_t *tiles = reinterpret_cast<uint32_t *>(ws + L.off_tiles);
    uint32_t *words = reinterpret_cast<uint32_t *>(ws + L.off_words);
    const uint32_t cap_words = (uint32_t)(L.unstuffed_bytes / 4);
    const int n_groups = (L.d.n_mcu + MCUS_PER_WG - 1) / MCUS_PER_WG;
    const uint32_t per_lane = (L.n_blocks + WG - 1) / WG, int_wgs = ((uint32_t)L.d.n_int + WG - 1) / WG;

    hipLaunchKernelGGL(jpeg_transform_kernel, dim3(grid_for(n_groups, n_workgroups, 4096)), dim3(WG), 0, st, rgb_hwc, L.d, quality, n_groups, coef);
    hipLaunchKernelGGL(jpeg_length_kernel, dim3(grid_for(per_lane, n_workgroups, 4096)), dim3(WG), 0, st, coef, (int)L.n_blocks, L.d.Ri, bits);
    exclusive_scan(bits, L.n_blocks, tiles, n_workgroups, st);
    hipLaunchKernelGGL(jpeg_interval_kernel, dim3(grid_for(int_wgs, n_workgroups, 1024)), dim3(WG), 0, st, bits, L.d, ibytes);
    exclusive_scan(ibytes, (uint32_t)L.d.n_int, tiles, n_workgroups, st);
    hipLaunchKernelGGL(jpeg_zero_kernel, dim3(grid_for(cap_words / WG + 1, n_workgroups, 1024)), dim3(WG), 0, st, ibytes, L.d.n_int, words, cap_words);
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3(grid_for(per_lane, n_workgroups, 4096)), dim3(WG), 0, st, coef, bits, ibytes, L.d, words, cap_words);
    hipLaunchKernelGGL(jpeg_count_kernel, dim3(grid_for(L.max_chunks / 4 + 1, n_workgroups, 1024)), dim3(WG), 0, st, words, ibytes, L.d.n_int,
                       L.max_chunks, ffc);
    exclusive_scan(ffc, L.max_chunks, tiles, n_workgroups, st);
    hipLaunchKernelGGL(jpeg_stuff_kernel, dim3(grid_for(L.max_chunks / 4 + 1, n_workgroups, 1024)), dim3(WG), 0, st, words, ibytes, ffc, L.d.n_int,
                       scan, (uint32_t)L.scan_bound, scan_bytes_dev);
    return sdn::check_launch("sdn_jpeg_encode_scan");
}

}  // extern "C"
