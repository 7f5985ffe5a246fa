// crt_bloom's kernels (bloom.hip): bright light of one of the scene's float images spread over an image pyramid and put
// back on the image.  Every float step is one IEEE float32 operation in the order include/crt.h writes, so a float32 numpy restatement
// (tests/bloom_ref.py) gives the same bits whatever the tiling.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crt {

constexpr uint32_t kBloomMaxLevels = 8;

// the input pixel and the bright pass
struct BloomSource {
    const float* image;          // width * height pixels of 3 floats, linear order
    uint32_t width, height;
    uint32_t scale;              // 1: c = image * inv_count (the running sum); 0: c = image
    float inv_count;
    float threshold, clamp;      // clamp 0 = none
};

// level 1 = Down(bright(c)): the scaling, the bright pass and the first filter in one launch; b is never stored
void launch_bloom_down_first(const BloomSource& src, float* d1, hipStream_t stream);
// level k = Down(level k - 1), w x h the size of level k - 1
void launch_bloom_down(const float* parent, uint32_t w, uint32_t h, float* child, hipStream_t stream);
// U_k = D_k + (Up(U_{k+1}) - D_k) * scatter, over D_k in place; w x h the size of level k, coarse = U_{k+1} of ((w + 1) >> 1) x ((h + 1) >> 1)
void launch_bloom_up(const float* coarse, float* level, uint32_t w, uint32_t h, float scatter, hipStream_t stream);
// out = c + (Up(U_1) - c) * strength (conserve) or c + Up(U_1) * strength: the last Up and the composite in one launch; G is never stored
void launch_bloom_composite(const BloomSource& src, const float* u1, uint32_t conserve, float strength, float* out, hipStream_t stream);
// out = c: a frame one pixel wide or high has no pyramid
void launch_bloom_copy(const BloomSource& src, float* out, hipStream_t stream);

}  // namespace crt
