// The deformer's kernel (deform.hip): linear blend skinning with four influences per element and morph targets on the
// positions, one thread per output element.  Every float step is host/deform_math.hpp's, which crt_deform_host runs on the CPU, so a
// float32 numpy restatement (tests/deform_ref.py) gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crt {

// the palette staged in LDS once per workgroup up to this many bones (48 B each: 12 KB, which leaves a CU's 160 KB room for 13
// workgroups of 4 waves, more than its 32 wave slots take); above it, and where the caller asks, bones come through the vector cache
constexpr uint32_t kDeformLdsBones = 256;
enum DeformPalette : int { kDeformPaletteAuto = 0, kDeformPaletteGlobal = 1, kDeformPaletteLds = 2 };

// one morph entry of a vertex's list: the delta and the target whose weight scales it
struct DeformMorph { float d[3]; uint32_t target; };

struct DeformArgs {
    // positions
    const float* rest_v;             // 3 per vertex
    const uint2* bones_v;            // four uint16 per vertex
    const float4* weights_v;
    const uint32_t* morph_first;     // n_vertices + 1 (entries of vertex v: [first[v], first[v + 1])), or null: no target lists anything
    const DeformMorph* morph;        // per vertex in ascending target order
    float* out_v;
    uint32_t n_vertices;
    // normals (n_normals may be 0)
    uint32_t n_normals;
    const float* rest_n;
    const uint2* bones_n;
    const float4* weights_n;
    float* out_n;
    // the pose: 3 float4 per bone, then the morph weights
    const float4* palette;
    const float* morph_weights;
    uint32_t n_bones;
};

// form: kDeformPaletteGlobal or kDeformPaletteLds (the latter only with n_bones <= kDeformLdsBones)
void launch_deform(const DeformArgs& a, int form, hipStream_t stream);

}  // namespace crt
