// Lossless PNG encoder (8-bit RGB, colour type 2, no interlace): the zlib stream of the IDAT chunk made on the device from the uint8
// [H,W,3] pixels `output.to_uint8_hwc` returns.  It replaces the Pillow encode of the per-frame PNG the reference writes (write_img,
// imaginaire/generators/scenedreamer.py:512-518, :629-631).  The host adds the signature, IHDR, the chunk framing with its CRC-32
// and IEND (png.py).
//
// The contract is the BYTES: all arithmetic is integer, tests/png_ref.py restates it in numpy and the two are compared with ==.
//
// FORMAT.  F = H rows of 1 + 3W bytes: the filter type, then the row filtered with bpp = 3 (a missing left pixel or prior row counts
// as zero, Avg floors, Paeth breaks ties a, b, c).  filter_mode 0 .. 4 forces the type; 5 takes per row the type with the smallest
// sum of (b < 128 ? b : 256 - b) over the filtered bytes, the smallest type on a tie.  Tokens are made per row: the filter byte is a
// literal; with e[j] = (r[j] == r[j - 1]) for j >= 1 over the payload r, every maximal run of e-true positions is cut from its front
// into pieces of 258; a piece of >= 3 is a match (length, distance 1), a last piece of 1 or 2 is literals.  One deflate block
// (BFINAL = 1, BTYPE = 10) holds the frame: the header, the tokens, symbol 256, zero bits up to the byte.  The stream is 78 01, the
// block, the Adler-32 of F (big-endian).
//
// THE BUILDER'S CHOICES (restated in tests/png_ref.py):
// LENGTHS (build_lengths: the literal/length code from the frame's histogram of symbols 0 .. 285 with symbol 256 counted once, limit
//   15; the code-length code, limit 7).  The used symbols (count > 0) are sorted ascending by (count, symbol).  A Huffman tree is built
//   with two queues, the sorted leaves and the internal nodes in the order they are made: each step takes the two smallest fronts, the
//   leaf queue winning a tie against the internal queue, and appends their sum.  n[d] = number of leaves at depth min(d, limit).
//   While sum n[d] 2^(limit - d) exceeds 2^limit: n[limit] -= 1; the largest d < limit with n[d] > 0 gives n[d] -= 1, n[d + 1] += 2
//   (each step lowers the sum by one unit and keeps the number of codes, so it ends at exactly 2^limit: a complete code).  The sorted
//   symbols then receive the lengths from the longest down: the first n[limit] get `limit`, the next n[limit - 1] get limit - 1, ...
//   A single used symbol gets length 1 (it cannot occur here: a frame has a literal and symbol 256; the length list has a 0 and the
//   distance's 1).  Codes are canonical (RFC 1951 3.2.2) and stored bit-reversed for deflate's LSB-first order.
// HEADER.  HLIT = max(257, 1 + the largest used symbol) - 257, HDIST = 0 (one distance code, symbol 0 with length 1, declared whether
//   or not a match occurs), HCLEN = 15 (all 19 code-length-code lengths are sent, 3 bits each).  The HLIT + 257 lengths and the one
//   distance length are each sent as their own code-length symbol 0 .. 15; symbols 16 - 18 are never used.
//   <= 17 + 57 + 7 * 287 = 2083 bits.
//
//   png_clear_kernel   zeroes the global histogram.
//   png_rows_kernel    one workgroup per row: the five scores and the choice, the row of F; then, from F, the bit mask of the
//                      positions with e false in LDS (one wave ballot per 64 positions), and per position its token (uint16: 0 = inside
//                      a match, 1 + v = literal v, 254 + n = match of n) found from the nearest set bits before and after it; symbols
//                      are counted in LDS with integer atomics and added to global memory with vector atomicAdd.
//   png_tree_kernel    one workgroup: ranks the symbols in parallel, merges on one lane (2 n steps), walks the leaves' depths in
//                      parallel, limits, assigns canonical codes in parallel, builds the header bit string with a workgroup scan.
//   png_cost_kernel    one workgroup per 256 positions of F: the bits of its tokens, and its Adler pair (sum d, sum (n - i) d).
//   scan_*_kernel      (int_scan.h, shared with jpeg.hip) exclusive prefix sum of the chunk bits.
//   png_zero_kernel    zeroes the words of the stream that this frame uses (the total is a device word).
//   png_pack_kernel    one workgroup per 256 positions: a workgroup scan gives every token its bit offset; code, extra bits and the
//                      distance bit are ORed into the stream with vector atomicOr (two words where the token straddles).
//   png_finish_kernel  one workgroup: 78 01, the header bits, symbol 256; the chunks' Adler pairs combined in row order
//                      (A' = A + a, B' = B + n A + b, 64-bit integers mod 65521; the operation is associative, so every lane folds a
//                      contiguous range and lane 0 folds the 256 results); the trailer and the byte count.
//
// Every loop over rows / chunks is a grid-stride loop and every sum an integer sum: the bytes do not depend on n_workgroups.
//
// SIZES.  A literal costs <= 15 bits for its position; a match costs <= 15 + 5 + 1 bits for >= 3 positions; symbol 256 <= 15 bits.
// sdn_png_stream_bound = ceil((15 (H (1 + 3W) + 1) + 2083) / 8) + 6 (78 01 and the Adler-32), rounded up to whole 32-bit words.  Bit
// offsets are uint32, so frames whose bound in bits does not fit 32 bits are refused (about 95 Mpixel).
//
// Stores to global memory are ordinary vector stores and vector atomics.  No float arithmetic.
#include "sdn_common.h"

namespace {

#include "int_scan.h"

constexpr int N_SYM = 286;
constexpr int MAX_ROW = 3 * 65535;                      // payload bytes of the widest row
constexpr int MASK_WORDS = (MAX_ROW / WG + 1) * (WG / 64);
constexpr uint32_t HEADER_FIXED_BITS = 17 + 3 * 19;
constexpr uint32_t HEADER_MAX_BITS = HEADER_FIXED_BITS + 7 * 287;
constexpr int HDR_WORDS = 68;                           // >= ceil(2083 / 32) + 1; word HDR_WORDS holds the header's bit count
constexpr uint32_t ADLER_MOD = 65521;

__constant__ constexpr uint8_t CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// RFC 1951 3.2.5: length symbol 257 + k stands for base[k] .. base[k] + 2^extra[k] - 1; k_of[n - 3] is the k of match length n
struct LenTable {
    uint16_t base[29];
    uint8_t extra[29];
    uint8_t k_of[256];
};
constexpr LenTable make_len_table() {
    constexpr uint16_t base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    constexpr uint8_t extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    LenTable t{};
    for (int k = 0; k < 29; k++) {
        t.base[k] = base[k];
        t.extra[k] = extra[k];
    }
    for (int n = 3; n <= 258; n++) {
        int k = 28;
        while (n < base[k]) k--;
        t.k_of[n - 3] = (uint8_t)k;
    }
    return t;
}
__constant__ LenTable c_len = make_len_table();

struct PngDims {
    int32_t H, W;
    uint32_t row_bytes;                                 // 1 + 3W
    uint32_t n_pos, n_chunks;                           // H * row_bytes, ceil(n_pos / 256)
};

// ---- filters ----------------------------------------------------------------------------------------------------------------------------
__device__ inline int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ inline int filter_byte(int type, int x, int a, int b, int c) {
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? ((a + b) >> 1) : paeth(a, b, c);
    return (x - pred) & 255;
}

__device__ inline uint32_t score_of(int v) { return (uint32_t)(v < 128 ? v : 256 - v); }

__global__ __launch_bounds__(WG) void png_clear_kernel(uint32_t *hist) {
    for (int i = threadIdx.x; i < N_SYM + 2; i += WG) hist[i] = 0u;
}

__global__ __launch_bounds__(WG) void png_rows_kernel(const uint8_t *rgb, PngDims d, int mode, uint8_t *F, uint16_t *tok, uint32_t *hist) {
    __shared__ uint64_t s_mask[MASK_WORDS];
    __shared__ uint32_t s_hist[N_SYM + 2];
    __shared__ uint32_t s_red[(WG / 64) * 5];
    __shared__ int s_type;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = 3 * d.W;
    for (int i = t; i < N_SYM + 2; i += WG) s_hist[i] = 0u;
    __syncthreads();
    for (int row = blockIdx.x; row < d.H; row += gridDim.x) {
        const uint8_t *cur = rgb + (size_t)row * n;
        const uint8_t *prior = cur - n;                 // read only where row > 0
        int type = mode;
        if (mode == 5) {
            uint32_t sums[5] = {0u, 0u, 0u, 0u, 0u};
            for (int j = t; j < n; j += WG) {
                const int x = cur[j], a = j >= 3 ? cur[j - 3] : 0, b = row > 0 ? prior[j] : 0, c = (row > 0 && j >= 3) ? prior[j - 3] : 0;
#pragma unroll
                for (int f = 0; f < 5; f++) sums[f] += score_of(filter_byte(f, x, a, b, c));
            }
#pragma unroll
            for (int f = 0; f < 5; f++) {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) sums[f] += __shfl_xor(sums[f], off, 64);
                if (lane == 0) s_red[wave * 5 + f] = sums[f];
            }
            __syncthreads();
            if (t == 0) {
                int best = 0;
                uint32_t best_sum = 0;
                for (int f = 0; f < 5; f++) {
                    uint32_t s = 0;
                    for (int w = 0; w < WG / 64; w++) s += s_red[w * 5 + f];
                    if (f == 0 || s < best_sum) {
                        best = f;
                        best_sum = s;
                    }
                }
                s_type = best;
            }
            __syncthreads();
            type = s_type;
        }
        uint8_t *Frow = F + (size_t)row * d.row_bytes;
        if (t == 0) Frow[0] = (uint8_t)type;
        for (int j = t; j < n; j += WG) {
            const int x = cur[j], a = j >= 3 ? cur[j - 3] : 0, b = row > 0 ? prior[j] : 0, c = (row > 0 && j >= 3) ? prior[j - 3] : 0;
            Frow[1 + j] = (uint8_t)filter_byte(type, x, a, b, c);
        }
        __syncthreads();                                // the row of F is visible to the workgroup
        // bit k of the mask: position k of the payload is a break (e[k] false); positions past the row count as breaks
        const uint8_t *r = Frow + 1;
        const int passes = n / WG + 1;                  // covers at least one position past the row
        for (int it = 0; it < passes; it++) {
            const int k = it * WG + t;
            const bool brk = k >= n || k == 0 || r[k] != r[k - 1];
            const uint64_t m = __ballot(brk);
            if (lane == 0) s_mask[it * (WG / 64) + wave] = m;
        }
        __syncthreads();
        uint16_t *trow = tok + (size_t)row * d.row_bytes;
        if (t == 0) {
            trow[0] = (uint16_t)(1 + type);
            atomicAdd(&s_hist[type], 1u);
        }
        for (int k = t; k < n; k += WG) {
            const int v = r[k];
            int wi = k >> 6;
            const uint64_t below = (2ull << (k & 63)) - 1ull;       // bits 0 .. k & 63
            uint64_t m = s_mask[wi];
            uint32_t token = 1u + (uint32_t)v;
            if (!((m >> (k & 63)) & 1ull)) {
                uint64_t mb = m & below;                // the break before k: it exists, bit 0 of word 0 is set
                int wb = wi;
                while (mb == 0ull && wb > 0) mb = s_mask[--wb];
                const int p = wb * 64 + 63 - __builtin_clzll(mb);
                uint64_t ma = m & ~below;               // the break after k: it exists, the position past the row is set
                int wa = wi;
                while (ma == 0ull && wa < passes * (WG / 64) - 1) ma = s_mask[++wa];
                const int nb = wa * 64 + __builtin_ctzll(ma);
                const int o = k - p - 1, L = nb - p - 1;
                const int piece = o / 258, q = o - piece * 258;
                const int plen = min(258, L - piece * 258);
                if (plen >= 3) token = q == 0 ? 254u + (uint32_t)plen : 0u;
            }
            trow[1 + k] = (uint16_t)token;
            if (token) atomicAdd(&s_hist[token <= 256u ? token - 1u : 257u + c_len.k_of[token - 257u]], 1u);
        }
        __syncthreads();                                // the mask is read; s_red and s_type may be written again
    }
    for (int i = t; i < N_SYM; i += WG)
        if (s_hist[i]) atomicAdd(&hist[i], s_hist[i]);
}

// ---- code construction --------------------------------------------------------------------------------------------------------------------
struct TreeLds {
    uint32_t cnt[N_SYM + 2];
    uint32_t w[2 * N_SYM];
    uint16_t par[2 * N_SYM];
    uint16_t order[N_SYM + 2];
    uint8_t len[N_SYM + 2];
    uint32_t code[N_SYM + 2];                           // (bit-reversed code << 8) | length
    int num[16], start[16], next[16];
    int n_used;
};

// s.cnt[0 .. n_sym) -> s.len, s.code (see LENGTHS above); called by the whole workgroup
__device__ void build_lengths(TreeLds &s, int n_sym, int limit) {
    const int t = threadIdx.x;
    if (t == 0) s.n_used = 0;
    if (t < 16) s.num[t] = 0;
    for (int sy = t; sy < n_sym; sy += WG) s.len[sy] = 0;
    __syncthreads();
    for (int sy = t; sy < n_sym; sy += WG) {
        const uint32_t c = s.cnt[sy];
        if (c) {
            int rank = 0;
            for (int u = 0; u < n_sym; u++) {
                const uint32_t cu = s.cnt[u];
                rank += (cu != 0u && (cu < c || (cu == c && u < sy))) ? 1 : 0;
            }
            s.w[rank] = c;
            s.order[rank] = (uint16_t)sy;
            atomicAdd(&s.n_used, 1);
        }
    }
    __syncthreads();
    const int n = s.n_used;
    if (n == 1 && t == 0) {
        s.len[s.order[0]] = 1;
        s.num[1] = 1;
    }
    if (n >= 2) {
        if (t == 0) {
            int li = 0, ii = n;
            for (int ni = n; ni < 2 * n - 1; ni++) {
                uint32_t sum = 0;
#pragma unroll
                for (int pick = 0; pick < 2; pick++) {
                    int x;
                    if (li < n && (ii >= ni || s.w[li] <= s.w[ii])) x = li++;
                    else x = ii++;
                    sum += s.w[x];
                    s.par[x] = (uint16_t)ni;
                }
                s.w[ni] = sum;
            }
        }
        __syncthreads();
        for (int leaf = t; leaf < n; leaf += WG) {
            int depth = 0, x = leaf;
            while (x != 2 * n - 2 && depth < 2 * N_SYM) {    // the root is 2 n - 2; a leaf is at most n - 1 below it
                x = s.par[x];
                depth++;
            }
            atomicAdd(&s.num[min(depth, limit)], 1);
        }
        __syncthreads();
        if (t == 0) {
            uint32_t total = 0;
            for (int dd = 1; dd <= limit; dd++) total += (uint32_t)s.num[dd] << (limit - dd);
            while (total > (1u << limit)) {
                s.num[limit]--;
                for (int dd = limit - 1; dd >= 1; dd--)
                    if (s.num[dd]) {
                        s.num[dd]--;
                        s.num[dd + 1] += 2;
                        break;
                    }
                total--;
            }
            int k = 0;
            for (int dd = limit; dd >= 1; dd--) {
                s.start[dd] = k;
                k += s.num[dd];
            }
        }
        __syncthreads();
        for (int rk = t; rk < n; rk += WG)
            for (int dd = 1; dd <= limit; dd++)
                if (rk >= s.start[dd] && rk < s.start[dd] + s.num[dd]) s.len[s.order[rk]] = (uint8_t)dd;
    }
    __syncthreads();
    if (t == 0) {                                       // RFC 1951 3.2.2: the first code of every length
        int code = 0;
        s.num[0] = 0;
        for (int b = 1; b <= 15; b++) {
            code = (code + s.num[b - 1]) << 1;
            s.next[b] = code;
            if (b == limit) break;
        }
    }
    __syncthreads();
    for (int sy = t; sy < n_sym; sy += WG) {
        const int l = s.len[sy];
        uint32_t out = 0;
        if (l) {
            int code = s.next[l];
            for (int u = 0; u < sy; u++) code += s.len[u] == l ? 1 : 0;
            out = ((__brev((uint32_t)code) >> (32 - l)) << 8) | (uint32_t)l;
        }
        s.code[sy] = out;
    }
    __syncthreads();
}

__device__ inline void lds_put_bits(uint32_t *words, uint32_t pos, uint32_t value, uint32_t nbits) {
    if (nbits == 0u) return;
    const uint64_t v = (uint64_t)value << (pos & 31u);
    atomicOr(&words[pos >> 5], (uint32_t)v);
    if ((pos & 31u) + nbits > 32u) atomicOr(&words[(pos >> 5) + 1u], (uint32_t)(v >> 32));
}

// hist -> codes[N_SYM] ((reversed code << 8) | length), hdr[0 .. HDR_WORDS) the header bit string from BFINAL on, hdr[HDR_WORDS] its bits
__global__ __launch_bounds__(WG) void png_tree_kernel(const uint32_t *hist, uint32_t *codes, uint32_t *hdr) {
    __shared__ TreeLds s;
    __shared__ uint8_t s_ll[N_SYM + 2];
    __shared__ uint32_t s_hdr[HDR_WORDS];
    __shared__ uint32_t s_buf[2 * WG];
    __shared__ int s_nlit;
    const int t = threadIdx.x;
    for (int sy = t; sy < N_SYM; sy += WG) s.cnt[sy] = sy == 256 ? 1u : hist[sy];
    if (t == 0) s_nlit = 257;
    for (int i = t; i < HDR_WORDS; i += WG) s_hdr[i] = 0u;
    __syncthreads();
    for (int sy = t; sy < N_SYM; sy += WG)
        if (s.cnt[sy]) atomicMax(&s_nlit, sy + 1);
    build_lengths(s, N_SYM, 15);
    for (int sy = t; sy < N_SYM; sy += WG) {
        codes[sy] = s.code[sy];
        s_ll[sy] = s.len[sy];
    }
    __syncthreads();
    const int nlit = s_nlit;
    for (int i = t; i < 19; i += WG) s.cnt[i] = 0u;
    __syncthreads();
    for (int i = t; i <= nlit; i += WG) atomicAdd(&s.cnt[i < nlit ? s_ll[i] : 1], 1u);
    __syncthreads();
    build_lengths(s, 19, 7);
    if (t == 0) {
        uint32_t pos = 0;
        lds_put_bits(s_hdr, pos, 1u, 1);                 pos += 1;   // BFINAL
        lds_put_bits(s_hdr, pos, 2u, 2);                 pos += 2;   // BTYPE = 10
        lds_put_bits(s_hdr, pos, (uint32_t)(nlit - 257), 5); pos += 5;
        lds_put_bits(s_hdr, pos, 0u, 5);                 pos += 5;   // HDIST
        lds_put_bits(s_hdr, pos, 15u, 4);                pos += 4;   // HCLEN
        for (int i = 0; i < 19; i++) {
            lds_put_bits(s_hdr, pos, s.len[CL_ORDER[i]], 3);
            pos += 3;
        }
    }
    uint32_t cl[2], nb = 0;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int i = 2 * t + j;
        cl[j] = i <= nlit ? s.code[i < nlit ? s_ll[i] : 1] : 0u;
        nb += cl[j] & 255u;
    }
    uint32_t total;
    uint32_t pos = HEADER_FIXED_BITS + wg_exclusive_scan(nb, s_buf, &total);
#pragma unroll
    for (int j = 0; j < 2; j++) {
        lds_put_bits(s_hdr, pos, cl[j] >> 8, cl[j] & 255u);
        pos += cl[j] & 255u;
    }
    __syncthreads();
    for (int i = t; i < HDR_WORDS; i += WG) hdr[i] = s_hdr[i];
    if (t == 0) hdr[HDR_WORDS] = HEADER_FIXED_BITS + total;
}

// ---- cost, pack, finish -------------------------------------------------------------------------------------------------------------------
__device__ inline void load_codes(uint32_t *s_code, const uint32_t *codes) {
    for (int i = threadIdx.x; i < N_SYM; i += WG) s_code[i] = codes[i];
    __syncthreads();
}

// token -> the bits it writes (value, LSB first) and their number (<= 15 + 5 + 1)
__device__ inline uint32_t token_bits(uint32_t token, const uint32_t *s_code, uint32_t *nbits) {
    if (token == 0u) {
        *nbits = 0u;
        return 0u;
    }
    if (token <= 256u) {
        const uint32_t c = s_code[token - 1u];
        *nbits = c & 255u;
        return c >> 8;
    }
    const uint32_t k = c_len.k_of[token - 257u], c = s_code[257u + k], l = c & 255u, ne = c_len.extra[k];
    *nbits = l + ne + 1u;                               // + the distance code "0"
    return (c >> 8) | ((token - 254u - c_len.base[k]) << l);
}

__global__ __launch_bounds__(WG) void png_cost_kernel(const uint8_t *F, const uint16_t *tok, const uint32_t *codes, PngDims d,
                                                      uint32_t *chunk_bits, uint2 *adler) {
    __shared__ uint32_t s_code[N_SYM + 2];
    __shared__ uint32_t s_red[(WG / 64) * 3];
    load_codes(s_code, codes);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (uint32_t ch = blockIdx.x; ch < d.n_chunks; ch += gridDim.x) {
        const uint32_t i = ch * WG + t, cnt = min((uint32_t)WG, d.n_pos - ch * WG);
        uint32_t v[3] = {0u, 0u, 0u};
        if (i < d.n_pos) {
            token_bits(tok[i], s_code, &v[0]);
            v[1] = F[i];
            v[2] = (cnt - (uint32_t)t) * v[1];
        }
#pragma unroll
        for (int f = 0; f < 3; f++) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v[f] += __shfl_xor(v[f], off, 64);
            if (lane == 0) s_red[wave * 3 + f] = v[f];
        }
        __syncthreads();
        if (t < 3) {
            uint32_t sum = 0;
            for (int w = 0; w < WG / 64; w++) sum += s_red[w * 3 + t];
            if (t == 0) chunk_bits[ch] = sum;
            if (t == 1) adler[ch].x = sum;              // <= 256 * 255
            if (t == 2) adler[ch].y = sum;              // <= 255 * 256 * 257 / 2
        }
        __syncthreads();
    }
}

// chunk_off: exclusive prefix of the chunk bits, n_chunks + 1 entries
__device__ inline uint32_t stream_bits(const uint32_t *chunk_off, const uint32_t *hdr, const uint32_t *codes, uint32_t n_chunks) {
    return 16u + hdr[HDR_WORDS] + chunk_off[n_chunks] + (codes[256] & 255u);
}

__global__ __launch_bounds__(WG) void png_zero_kernel(const uint32_t *chunk_off, const uint32_t *hdr, const uint32_t *codes, uint32_t n_chunks,
                                                      uint32_t *words, uint32_t cap_words) {
    const uint32_t bytes = ((stream_bits(chunk_off, hdr, codes, n_chunks) + 7u) >> 3) + 4u;
    const uint32_t n = min((bytes + 3u) >> 2, cap_words);
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) words[i] = 0u;
}

__device__ inline void put_bits(uint32_t *words, uint32_t cap_words, uint32_t pos, uint32_t value, uint32_t nbits) {
    if (nbits == 0u) return;
    const uint64_t v = (uint64_t)value << (pos & 31u);
    const uint32_t w = pos >> 5;
    if (w < cap_words) atomicOr(&words[w], (uint32_t)v);
    if ((pos & 31u) + nbits > 32u && w + 1u < cap_words) atomicOr(&words[w + 1u], (uint32_t)(v >> 32));
}

__global__ __launch_bounds__(WG) void png_pack_kernel(const uint16_t *tok, const uint32_t *codes, const uint32_t *chunk_off, const uint32_t *hdr,
                                                      PngDims d, uint32_t *words, uint32_t cap_words) {
    __shared__ uint32_t s_code[N_SYM + 2];
    __shared__ uint32_t s_buf[2 * WG];
    load_codes(s_code, codes);
    const uint32_t base = 16u + hdr[HDR_WORDS];
    for (uint32_t ch = blockIdx.x; ch < d.n_chunks; ch += gridDim.x) {
        const uint32_t i = ch * WG + threadIdx.x;
        uint32_t nbits = 0u, value = 0u;
        if (i < d.n_pos) value = token_bits(tok[i], s_code, &nbits);
        uint32_t total;
        const uint32_t excl = wg_exclusive_scan(nbits, s_buf, &total);
        put_bits(words, cap_words, base + chunk_off[ch] + excl, value, nbits);
    }
}

__global__ __launch_bounds__(WG) void png_finish_kernel(const uint32_t *codes, const uint32_t *chunk_off, const uint32_t *hdr, const uint2 *adler,
                                                        PngDims d, uint32_t *words, uint32_t cap_words, uint32_t *out_bytes) {
    __shared__ uint32_t s_n[WG], s_a[WG], s_b[WG];
    const int t = threadIdx.x;
    const uint32_t hdr_bits = hdr[HDR_WORDS];
    for (int i = t; i < HDR_WORDS; i += WG) put_bits(words, cap_words, 16u + 32u * (uint32_t)i, hdr[i], 32u);
    // this lane's contiguous range of chunks, folded from (n, a, b) = (0, 0, 0)
    const uint32_t per = (d.n_chunks + WG - 1) / WG;
    const uint32_t c0 = min((uint32_t)t * per, d.n_chunks), c1 = min(c0 + per, d.n_chunks);
    uint64_t n = 0, a = 0, b = 0;
    for (uint32_t ch = c0; ch < c1; ch++) {
        const uint64_t cnt = min((uint32_t)WG, d.n_pos - ch * WG);
        const uint2 p = adler[ch];
        b = (b + cnt * a + p.y) % ADLER_MOD;
        a = (a + p.x) % ADLER_MOD;
        n += cnt;
    }
    s_n[t] = (uint32_t)(n % ADLER_MOD);
    s_a[t] = (uint32_t)a;
    s_b[t] = (uint32_t)b;
    __syncthreads();
    if (t == 0) {
        uint64_t A = 1, B = 0;
        for (int i = 0; i < WG; i++) {
            B = (B + (uint64_t)s_n[i] * A + s_b[i]) % ADLER_MOD;
            A = (A + s_a[i]) % ADLER_MOD;
        }
        put_bits(words, cap_words, 0u, 0x0178u, 16u);   // 78 01: deflate, 32 K window, no dictionary, level 0; 0x7801 = 31 * 991
        const uint32_t eob = codes[256], end = 16u + hdr_bits + chunk_off[d.n_chunks];
        put_bits(words, cap_words, end, eob >> 8, eob & 255u);
        const uint32_t tail = (end + (eob & 255u) + 7u) >> 3;
        const uint32_t sum = (uint32_t)((B << 16) | A);
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) put_bits(words, cap_words, (tail + j) * 8u, (sum >> (24u - 8u * j)) & 255u, 8u);
        *out_bytes = tail + 4u;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
struct Layout {  // of the workspace, every part 256-byte aligned
    PngDims d;
    size_t bound;
    uint32_t max_tiles;
    size_t off_F, off_tok, off_hist, off_codes, off_hdr, off_bits, off_adler, off_tiles, total;
};

// false: the frame is outside what the encoder takes (sizes, or a bound whose bits do not fit 32 bits)
bool make_layout(int H, int W, Layout &L) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535) return false;
    const uint64_t row = 1 + 3ull * (uint64_t)W, n = row * (uint64_t)H;
    const uint64_t bits = 15ull * (n + 1) + HEADER_MAX_BITS;
    if (bits + 48 + 64 >= (1ull << 32)) return false;
    L.bound = (size_t)((((bits + 7) / 8 + 6) + 3) & ~3ull);
    L.d = PngDims{H, W, (uint32_t)row, (uint32_t)n, (uint32_t)((n + WG - 1) / WG)};
    L.max_tiles = (L.d.n_chunks + 1 + SCAN_TILE - 1) / SCAN_TILE;
    size_t o = 0;
    L.off_F = o;     o += align256((size_t)n);
    L.off_tok = o;   o += align256((size_t)n * 2);
    L.off_hist = o;  o += align256((N_SYM + 2) * 4);
    L.off_codes = o; o += align256((N_SYM + 2) * 4);
    L.off_hdr = o;   o += align256((HDR_WORDS + 1) * 4);
    L.off_bits = o;  o += align256(((size_t)L.d.n_chunks + 1) * 4);
    L.off_adler = o; o += align256((size_t)L.d.n_chunks * 8);
    L.off_tiles = o; o += align256(((size_t)L.max_tiles + 1) * 4);
    L.total = o;
    return true;
}

}  // namespace

extern "C" {

size_t sdn_png_stream_bound(int H, int W) {
    Layout L;
    return make_layout(H, W, L) ? L.bound : 0;
}

size_t sdn_png_workspace_bytes(int H, int W) {
    Layout L;
    return make_layout(H, W, L) ? L.total : 0;
}

int sdn_png_encode(const uint8_t *rgb_hwc, int H, int W, int filter_mode, void *workspace, uint8_t *zstream, uint32_t *zbytes_dev,
                   int n_workgroups, sdn_stream_t stream) {
    if (filter_mode < 0 || filter_mode > 5) return sdn::fail(SDN_ERR_UNSUPPORTED, "sdn_png_encode: filter_mode must be 0 .. 5 (got %d)", filter_mode);
    if (H < 0 || W < 0 || H > 65535 || W > 65535)
        return sdn::fail(SDN_ERR_UNSUPPORTED, "sdn_png_encode: H and W must be 1 .. 65535 (got %d x %d)", H, W);
    if (H == 0 || W == 0) return SDN_OK;            // empty frame: nothing to encode
    if (!rgb_hwc || !workspace || !zstream || !zbytes_dev) return sdn::fail(SDN_ERR_UNSUPPORTED, "sdn_png_encode: null pointer");
    Layout L;
    if (!make_layout(H, W, L))
        return sdn::fail(SDN_ERR_UNSUPPORTED, "sdn_png_encode: %d x %d is too large: the stream's bit count does not fit 32 bits", H, W);
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    uint8_t *F = reinterpret_cast<uint8_t *>(ws + L.off_F);
    uint16_t *tok = reinterpret_cast<uint16_t *>(ws + L.off_tok);
    uint32_t *hist = reinterpret_cast<uint32_t *>(ws + L.off_hist);
    uint32_t *codes = reinterpret_cast<uint32_t *>(ws + L.off_codes);
    uint32_t *hdr = reinterpret_cast<uint32_t *>(ws + L.off_hdr);
    uint32_t *bits = reinterpret_cast<uint32_t *>(ws + L.off_bits);
    uint2 *adler = reinterpret_cast<uint2 *>(ws + L.off_adler);
    uint32_t *tiles = reinterpret_cast<uint32_t *>(ws + L.off_tiles);
    uint32_t *words = reinterpret_cast<uint32_t *>(zstream);
    const uint32_t cap_words = (uint32_t)(L.bound / 4);
    const unsigned chunk_grid = grid_for(L.d.n_chunks, n_workgroups, 8192);

    hipLaunchKernelGGL(png_clear_kernel, dim3(1), dim3(WG), 0, st, hist);
    hipLaunchKernelGGL(png_rows_kernel, dim3(grid_for((uint64_t)H, n_workgroups, 4096)), dim3(WG), 0, st, rgb_hwc, L.d, filter_mode, F, tok, hist);
    hipLaunchKernelGGL(png_tree_kernel, dim3(1), dim3(WG), 0, st, hist, codes, hdr);
    hipLaunchKernelGGL(png_cost_kernel, dim3(chunk_grid), dim3(WG), 0, st, F, tok, codes, L.d, bits, adler);
    exclusive_scan(bits, L.d.n_chunks, tiles, n_workgroups, st);
    hipLaunchKernelGGL(png_zero_kernel, dim3(grid_for(cap_words / WG + 1, n_workgroups, 1024)), dim3(WG), 0, st, bits, hdr, codes, L.d.n_chunks, words,
                       cap_words);
    hipLaunchKernelGGL(png_pack_kernel, dim3(chunk_grid), dim3(WG), 0, st, tok, codes, bits, hdr, L.d, words, cap_words);
    hipLaunchKernelGGL(png_finish_kernel, dim3(1), dim3(WG), 0, st, codes, bits, hdr, adler, L.d, words, cap_words, zbytes_dev);
    return sdn::check_launch("sdn_png_encode");
}

}  // extern "C"
