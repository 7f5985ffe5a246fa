// crt_display's kernels (display.hip): the display transform of one of the scene's three float images.  k_display_hist
// bins the image's luminance into 256 integer counts, k_display_meter turns the counts into an exposure and writes the state block,
// k_display applies exposure, tone curve and the pinned gamma.  Every float step is one IEEE float32 operation in a fixed order and the
// meter is integer arithmetic, so a float32 numpy restatement (tests/display_ref.py) gives the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crt.h"
#include "rt_kernels.hpp"

namespace crt {

// The state block in device memory, 8 words.  Words 0..4 are crt_display_state's; word 5 is the adapted exposure, which a manual call
// leaves alone (word 0 is the exposure of the LAST call, manual or not).
enum { kDisplayExposure = 0, kDisplayMetered = 1, kDisplayCounted = 2, kDisplayQ = 3, kDisplayCalls = 4, kDisplayAdapted = 5, kDisplayStateWords = 8 };

// The live bins are kept kDisplayBinCopies times over and a workgroup of k_display_hist adds to copy blockIdx.x % kDisplayBinCopies: its
// 2,048 workgroups otherwise queue up on 256 addresses of one L2 channel.  Integer sums: the total does not depend on who added where.
constexpr uint32_t kDisplayBinCopies = 16;
// one allocation: the state block, the live bins, the bins as last metered
constexpr uint32_t kDisplayBinsAt = kDisplayStateWords, kDisplayLastAt = kDisplayBinsAt + 256u * kDisplayBinCopies, kDisplayWords = kDisplayLastAt + 256u;

struct DisplayMeterArgs {
    uint32_t* bins;              // [kDisplayBinCopies][256] the live counts: summed over the copies, then zeroed for the next call
    uint32_t* last;              // [256] out: the counts as metered, before trimming
    uint32_t* state;             // [kDisplayStateWords]
    uint32_t metered;            // 0: a manual call, E = exposure and the adaptation words stay; bins and last are not touched
    float exposure;              // params.exposure
    float key, adapt, exposure_min, exposure_max;
    uint32_t low_permille, high_permille;
};

// one slice of the image: a packed tile buffer with its FrameArgs (the running sum), or width * height pixels in linear order
struct DisplaySlice {
    FrameArgs f;                 // packed only
    const float* image;          // 3 floats per pixel
    uint32_t n_pixels;           // linear only
    uint32_t packed;
    uint32_t grid;
};

// a packed slice is the running sum, c = image * inv_count; a linear one is taken as it is, c = image
void launch_display_hist(const DisplaySlice& sl, float inv_count, uint32_t* bins, hipStream_t stream);
void launch_display_meter(const DisplayMeterArgs& a, hipStream_t stream);
// curve: CRT_DISPLAY_CURVE_*; w2 = white * white for REINHARD; E is read from state[kDisplayExposure]
void launch_display(const DisplaySlice& sl, float inv_count, uint32_t curve, float w2, const uint32_t* state, const float* thr, uint8_t* rgba,
                    hipStream_t stream);

}  // namespace crt
