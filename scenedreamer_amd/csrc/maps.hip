// Depth and opacity maps of a frame, made from the two per-sample arrays the field kernels already write (sdn_field_aux.weights /
// .depth): the tail of Generator.inference_givenstyle_depth (imaginaire/generators/scenedreamer.py:636-851) -- the compositing of
// :816, the crop of :821-823, the normalisation over the pixels that hit something of :835-841 and the 8-bit values cv2.imwrite
// stores at :844.  Nothing here touches the field kernels: the maps are a function of the aux arrays alone.
//
// The contract is the BITS: tests/depth_maps_ref.py restates the arithmetic in numpy and the two are compared with ==.
//
// ARITHMETIC (fixed).
//   compositing  per kept ray: acc = 0.0 (f64); for s ascending acc += (double)w[s] * (double)z[s] (the product of two f32 values is
//                exact in f64, so a fused multiply-add would give the same bits); depth_map = (float)acc, ONE rounding -- the rule of
//                world_f32.hip's tail and style kernels.  opacity: the same accumulation over w[s] alone.
//   range        the f32 bit patterns of the smallest and the largest depth_map value that is > 0 and finite.  Positive floats order
//                as their unsigned bit patterns, so the reduction is an integer min / max: per lane over its rays, a wave reduction, a
//                workgroup reduction in LDS, one vector atomicMin / atomicMax on unsigned int per workgroup.  Min and max do not depend
//                on the order: no bit depends on the launch shape.  No float atomics.  The pair is initialised by a clear launch of
//                this entry on the same stream to {0x7F800000, 0}: range[1] == 0 means "no pixel hit anything".
//   quantise     for d > 0 and finite: t = (d - lo) / (hi - lo) in f32, a correctly rounded division; t = 0 when hi == lo; t clamped
//                to [0, 1] (a NaN t, which only a caller-made range can produce, counts as 0); v = rintf(t * (2^bits - 1)), ties to
//                even.  The rounding rule is OpenCV's documented saturate_cast<uchar>(float) of convertTo (round to nearest, ties to
//                even), which is what imwrite applies to the float image of :844; it was taken from the documentation, not measured
//                against an OpenCV build.  Every other d, NaN included: 2^bits - 1 (`fake_depth[~mmask] = 1`, :840).
//
//   maps_clear_kernel      one lane: the range pair.
//   depth_maps_kernel<V4>  one lane per kept pixel, grid-stride; V4 (num_samples % 4 == 0 and both arrays 16-byte aligned: every row is
//                          then) reads the two rows as float4, otherwise element by element.  The same sums in the same order.
//   depth_quantise_kernel<T>  one lane per pixel, grid-stride; T = uint8_t / uint16_t.
//
// Stores to global memory are ordinary vector stores and vector atomics.  Compiled with -ffp-contract=off.
#include "sdn_common.h"

#include <climits>

namespace {

constexpr int WG = 256;
constexpr uint32_t RANGE_LO_INIT = 0x7F800000u;         // +inf: above every finite positive pattern
constexpr uint32_t RANGE_HI_INIT = 0u;

__global__ void maps_clear_kernel(uint32_t *range_bits) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        range_bits[0] = RANGE_LO_INIT;
        range_bits[1] = RANGE_HI_INIT;
    }
}

template <bool V4>
__global__ __launch_bounds__(WG) void depth_maps_kernel(const float *__restrict__ weights, const float *__restrict__ sample_depth, int cols,
                                                        int num_samples, int crop, int out_cols, int64_t n_out, float *__restrict__ depth_map,
                                                        float *__restrict__ opacity, uint32_t *range_bits) {
    __shared__ uint32_t s_lo[WG / 64], s_hi[WG / 64];
    uint32_t lo = RANGE_LO_INIT, hi = RANGE_HI_INIT;
    for (int64_t p = (int64_t)blockIdx.x * WG + threadIdx.x; p < n_out; p += (int64_t)gridDim.x * WG) {
        const int64_t y = p / out_cols, x = p - y * out_cols;
        const int64_t ray = (y + crop) * cols + (x + crop);
        const float *w = weights + ray * num_samples, *z = sample_depth + ray * num_samples;
        double acc = 0.0, op = 0.0;
        if (V4) {
            const float4 *w4 = reinterpret_cast<const float4 *>(w), *z4 = reinterpret_cast<const float4 *>(z);
            for (int q = 0; q < num_samples / 4; q++) {
                const float4 a = w4[q], b = z4[q];
                acc += (double)a.x * (double)b.x;
                acc += (double)a.y * (double)b.y;
                acc += (double)a.z * (double)b.z;
                acc += (double)a.w * (double)b.w;
                op += (double)a.x;
                op += (double)a.y;
                op += (double)a.z;
                op += (double)a.w;
            }
        } else {
            for (int s = 0; s < num_samples; s++) {
                const float a = w[s];
                acc += (double)a * (double)z[s];
                op += (double)a;
            }
        }
        const float d = (float)acc;
        depth_map[p] = d;
        if (opacity) opacity[p] = (float)op;
        const uint32_t b = __float_as_uint(d);
        if (d > 0.f && b < RANGE_LO_INIT) {              // positive and finite (NaN fails d > 0)
            lo = b < lo ? b : lo;
            hi = b > hi ? b : hi;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t l2 = __shfl_xor(lo, off, 64), h2 = __shfl_xor(hi, off, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0) {
        s_lo[threadIdx.x >> 6] = lo;
        s_hi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < WG / 64; i++) {
            lo = s_lo[i] < lo ? s_lo[i] : lo;
            hi = s_hi[i] > hi ? s_hi[i] : hi;
        }
        if (hi != RANGE_HI_INIT) {                      // (lo and hi are set together)
            atomicMin(&range_bits[0], lo);
            atomicMax(&range_bits[1], hi);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(WG) void depth_quantise_kernel(const float *__restrict__ depth_map, int64_t n, const uint32_t *__restrict__ range_bits,
                                                            float top, T *__restrict__ out) {
    const float lo = __uint_as_float(range_bits[0]), hi = __uint_as_float(range_bits[1]);
    const float span = hi - lo;
    for (int64_t p = (int64_t)blockIdx.x * WG + threadIdx.x; p < n; p += (int64_t)gridDim.x * WG) {
        const float d = depth_map[p];
        float v = top;
        if (d > 0.f && __float_as_uint(d) < RANGE_LO_INIT) {
            float t = hi == lo ? 0.f : __fdiv_rn(d - lo, span);
            t = t > 0.f ? t : 0.f;                       // (NaN -> 0)
            t = t < 1.f ? t : 1.f;
            v = rintf(t * top);
        }
        out[p] = (T)v;
    }
}

inline unsigned grid_for(int64_t items, int n_workgroups) {
    const int64_t want = n_workgroups > 0 ? n_workgroups : 256;      // one per CU
    const int64_t need = (items + WG - 1) / WG;
    return (unsigned)(need < 1 ? 1 : (need < want ? need : want));
}

}  // namespace

extern "C" {

int sdn_depth_maps(const float *weights, const float *sample_depth, int rows, int cols, int num_samples, int crop, float *depth_map,
                   float *opacity, uint32_t *range_bits, int n_workgroups, sdn_stream_t stream) {
    SDN_REQUIRE(weights && sample_depth && depth_map && range_bits, "sdn_depth_maps: null pointer");
    SDN_REQUIRE(rows >= 1 && cols >= 1, "sdn_depth_maps: rows and cols must be >= 1 (got %d x %d)", rows, cols);
    SDN_REQUIRE(num_samples >= 1, "sdn_depth_maps: num_samples must be >= 1 (got %d)", num_samples);
    SDN_REQUIRE(crop >= 0, "sdn_depth_maps: crop must be >= 0 (got %d)", crop);
    SDN_REQUIRE(2 * (int64_t)crop < rows && 2 * (int64_t)crop < cols, "sdn_depth_maps: a crop of %d leaves nothing of %d x %d", crop, rows, cols);
    SDN_REQUIRE((int64_t)rows * cols * num_samples <= INT32_MAX, "sdn_depth_maps: %d x %d rays of %d samples are beyond int32", rows, cols,
                num_samples);
    const int out_cols = cols - 2 * crop;
    const int64_t n_out = (int64_t)(rows - 2 * crop) * out_cols;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(grid_for(n_out, n_workgroups));
    hipLaunchKernelGGL(maps_clear_kernel, dim3(1), dim3(64), 0, st, range_bits);
    const bool v4 = num_samples % 4 == 0 && ((reinterpret_cast<uintptr_t>(weights) | reinterpret_cast<uintptr_t>(sample_depth)) & 15) == 0;
    if (v4)
        hipLaunchKernelGGL(depth_maps_kernel<true>, grid, dim3(WG), 0, st, weights, sample_depth, cols, num_samples, crop, out_cols, n_out, depth_map,
                           opacity, range_bits);
    else
        hipLaunchKernelGGL(depth_maps_kernel<false>, grid, dim3(WG), 0, st, weights, sample_depth, cols, num_samples, crop, out_cols, n_out, depth_map,
                           opacity, range_bits);
    return sdn::check_launch("sdn_depth_maps");
}

int sdn_depth_quantise(const float *depth_map, int64_t n, const uint32_t *range_bits, int bits, void *out, int n_workgroups,
                       sdn_stream_t stream) {
    SDN_REQUIRE(depth_map && range_bits && out, "sdn_depth_quantise: null pointer");
    SDN_REQUIRE(n >= 1, "sdn_depth_quantise: n must be >= 1 (got %lld)", (long long)n);
    SDN_REQUIRE(n <= INT32_MAX, "sdn_depth_quantise: %lld pixels are beyond int32", (long long)n);
    SDN_REQUIRE(bits == 8 || bits == 16, "sdn_depth_quantise: bits must be 8 or 16 (got %d)", bits);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(grid_for(n, n_workgroups));
    if (bits == 8)
        hipLaunchKernelGGL(depth_quantise_kernel<uint8_t>, grid, dim3(WG), 0, st, depth_map, n, range_bits, 255.f, static_cast<uint8_t *>(out));
    else
        hipLaunchKernelGGL(depth_quantise_kernel<uint16_t>, grid, dim3(WG), 0, st, depth_map, n, range_bits, 65535.f, static_cast<uint16_t *>(out));
    return sdn::check_launch("sdn_depth_quantise");
}

}  // extern "C"
