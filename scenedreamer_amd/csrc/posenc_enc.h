// One degree of voxlib.positional_encoding for one value (imaginaire/model_utils/gancraft/voxlib/positional_encoding_kernel.cu:
// 63-66): sin and cos of x * pi_f * 2^d.  ONE definition for the op (posenc.hip) and for the kernels that evaluate the encoding
// themselves and promise the op's bits (sky_f32.hip), per translation unit like the other device headers.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr float kPiF = 3.141592654f;  // CUDART_PI_F

__device__ __forceinline__ void posenc_sincos(float x, int d, float &s, float &c) {
    const float rad = x * kPiF * exp2f((float)d);
    sincosf(rad, &s, &c);
}

}  // namespace
