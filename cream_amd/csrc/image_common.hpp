// image_common.hpp — what the input-transform kernels (image_transform.hip) and the RandAugment kernels (image_augment.hip) share:
// the float tail ToTensor -> Normalize (-> mirror) -> RandomErasing of four output pixels, and the host glue between the two files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cream_amd.h"

namespace cream_image {
typedef float f32x4 __attribute__((ext_vector_type(4)));

// standard-normal noise of RandomErasing's 'pixel' mode: two 32-bit counter-based hashes of (seed, channel, row, column) through
// Box-Muller (autoformer/data.py: erase_noise_reference restates it)
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
__device__ __forceinline__ float erase_noise(uint32_t seed, int c, int y, int x) {
    const uint32_t key = mix32(seed ^ ((uint32_t)(c + 1) * 0x9E3779B9u));
    const uint32_t h1 = mix32(key ^ (((uint32_t)y << 16) | (uint32_t)x));
    const uint32_t h2 = mix32(h1 ^ 0x85EBCA6Bu);
    const float u1 = ((float)(h1 >> 8) + 1.0f) * (1.0f / 16777216.0f);          // (0, 1]
    const float u2 = (float)(h2 >> 8) * (1.0f / 16777216.0f);                   // [0, 1)
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

// The float tail of four consecutive pixels of output row yo: u8[3 px + c] = channel c of pixel px (px = 0..3 left to right in the
// uint8 image), written to columns xo .. xo + 3 of the three planes at ob (+ c * plane), reversed when `flip`.
// torchvision F.to_tensor: float(v) / 255; F.normalize: (x - mean) / std — two IEEE float32 divisions, no contraction.
__device__ __forceinline__ void store_normalized4(float* ob, int64_t plane, int xo, int yo, bool flip, const int (&u8)[12],
                                                  const float (&mean)[3], const float (&sd)[3], const cream_image_desc& d) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        f32x4 v;
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            const float x = (float)u8[3 * px + c] / 255.f;
            v[flip ? 3 - px : px] = (x - mean[c]) / sd[c];
        }
        if (d.erase_h > 0 && yo >= d.erase_top && yo < d.erase_top + d.erase_h) {      // RandomErasing, mode 'pixel'
#pragma unroll
            for (int px = 0; px < 4; ++px)
                if (xo + px >= d.erase_left && xo + px < d.erase_left + d.erase_w) v[px] = erase_noise(d.erase_seed, c, yo, xo + px);
        }
        *reinterpret_cast<f32x4*>(ob + (int64_t)c * plane + xo) = v;
    }
}

// ---- host glue (image_augment.hip) -----------------------------------------------------------------------------------------------
int check_aug_ops(const cream_aug_op* ops, int64_t count);                  // CREAM_OK or CREAM_ERR_BAD_ARG
// Enqueue the op layers of a batch of RGBX images (one uint32 per pixel, R | G << 8 | B << 16; B images of H x W, packed) at
// `img`, ping-ponging through `img2` (unused when ops_per_image == 1); the last layer writes the float tail into out
// (B, 3, H, W) with the descriptors' RandomErasing boxes.
int launch_aug_tail(float* out, uint32_t* img, uint32_t* img2, const cream_aug_op* ops_dev, int ops_per_image, int B, int H, int W,
                    const cream_image_desc* descs_dev, const float* mean, const float* stdev, hipStream_t st);
}  // namespace cream_image
