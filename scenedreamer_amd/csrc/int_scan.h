// Exclusive prefix sums of uint32 arrays (modulo 2^32) and the launch helpers of the integer coders (csrc/jpeg.hip, csrc/png.hip):
// tile sums, one workgroup over the tile sums, apply.  Every sum is an integer sum and every loop over tiles is a grid-stride loop,
// so no value depends on the launch shape.  Included inside each file's own anonymous namespace.
#pragma once

constexpr int WG = 256;
constexpr int SCAN_TILE = 1024;                 // 256 threads x 4 elements

__device__ inline uint32_t wg_exclusive_scan(uint32_t v, uint32_t *s_buf, uint32_t *total) {  // s_buf: 2 * WG words
    const int t = threadIdx.x;
    int cur = 0;
    s_buf[t] = v;
    __syncthreads();
#pragma unroll 1
    for (int off = 1; off < WG; off <<= 1) {
        const uint32_t add = t >= off ? s_buf[cur * WG + t - off] : 0u;
        s_buf[(cur ^ 1) * WG + t] = s_buf[cur * WG + t] + add;
        cur ^= 1;
        __syncthreads();
    }
    const uint32_t incl = s_buf[cur * WG + t];
    *total = s_buf[cur * WG + WG - 1];
    __syncthreads();                                // s_buf may be written again
    return incl - v;
}

__global__ __launch_bounds__(WG) void scan_tile_sums_kernel(const uint32_t *in, uint32_t n, uint32_t n_tiles, uint32_t *tile_sums) {
    __shared__ uint32_t s_buf[2 * WG];
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t i0 = tile * SCAN_TILE + threadIdx.x * 4;
        uint32_t v = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) v += (i0 + j < n) ? in[i0 + j] : 0u;
        uint32_t total;
        wg_exclusive_scan(v, s_buf, &total);
        if (threadIdx.x == 0) tile_sums[tile] = total;
    }
}

// one workgroup: tile_sums -> exclusive tile offsets in place; the grand total to out_total
__global__ __launch_bounds__(WG) void scan_tile_offsets_kernel(uint32_t *tile_sums, uint32_t n_tiles, uint32_t *out_total) {
    __shared__ uint32_t s_buf[2 * WG];
    uint32_t base = 0;
    for (uint32_t i0 = 0; i0 < n_tiles; i0 += WG) {
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t v = i < n_tiles ? tile_sums[i] : 0u;
        uint32_t total;
        const uint32_t excl = wg_exclusive_scan(v, s_buf, &total);
        if (i < n_tiles) tile_sums[i] = base + excl;
        base += total;
    }
    if (threadIdx.x == 0) *out_total = base;
}

// in place: data[i] becomes the sum of the elements before i (data[n] was written by scan_tile_offsets_kernel)
__global__ __launch_bounds__(WG) void scan_apply_kernel(uint32_t *data, uint32_t n, uint32_t n_tiles, const uint32_t *tile_offsets) {
    __shared__ uint32_t s_buf[2 * WG];
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t i0 = tile * SCAN_TILE + threadIdx.x * 4;
        uint32_t e[4], v = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            e[j] = (i0 + j < n) ? data[i0 + j] : 0u;
            v += e[j];
        }
        uint32_t total;
        uint32_t run = tile_offsets[tile] + wg_exclusive_scan(v, s_buf, &total);
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            if (i0 + j < n) data[i0 + j] = run;
            run += e[j];
        }
    }
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

inline unsigned grid_for(uint64_t items, int n_workgroups, unsigned dflt) {
    const uint64_t want = n_workgroups > 0 ? (uint64_t)n_workgroups : (uint64_t)dflt;
    return (unsigned)(items < 1 ? 1 : (items < want ? items : want));
}

// data[0 .. n] <- exclusive prefix sums of data[0 .. n - 1], data[n] the total
inline void exclusive_scan(uint32_t *data, uint32_t n, uint32_t *tiles, int n_workgroups, hipStream_t st) {
    const uint32_t n_tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    const unsigned grid = grid_for(n_tiles, n_workgroups, 1024);
    hipLaunchKernelGGL(scan_tile_sums_kernel, dim3(grid), dim3(WG), 0, st, data, n, n_tiles, tiles);
    hipLaunchKernelGGL(scan_tile_offsets_kernel, dim3(1), dim3(WG), 0, st, tiles, n_tiles, data + n);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(grid), dim3(WG), 0, st, data, n, n_tiles, tiles);
}
