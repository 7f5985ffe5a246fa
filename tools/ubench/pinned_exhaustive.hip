// The LEAN forms of pinned_sin / pinned_cos (rt_math.hpp: the range test on the float, the parity from (int)k, the sign flipped after the
// rounding to float) against the bodies every other kernel keeps: 2^24 inputs, bit patterns compared.
//   - every binary exponent from 2^-30 to 2^30, both signs, random mantissas (what is left of the 2^24 after the lists below)
//   - +-0, +-inf, a NaN of either sign, the 64 floats on each side of +-1e9 (where the range test flips)
//   - the 4,096 floats nearest to k pi and to -k pi for k = 1 .. 64 (where the reduced argument passes through zero)
//   - the 4,096 floats nearest to +-(k + 1/2) pi for k = 0 .. 63 (where rint(x / pi) steps to the next integer, i.e. its parity flips)
// Prints the number of inputs on which each function's two forms differ, and a few of them.
// build: hipcc -O3 -ffp-contract=off --offload-arch=gfx950 -I caitlynrenderer_amd/csrc -o pinned_exhaustive tools/ubench/pinned_exhaustive.hip
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "rt_math.hpp"

__global__ void k_check(const uint32_t* in, uint32_t n, unsigned long long* counts, uint32_t* samples) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t bits = in[i];
        const float x = __uint_as_float(bits);
        const uint32_t s0 = __float_as_uint(crt::pinned_sin<false>(x)), s1 = __float_as_uint(crt::pinned_sin<true>(x));
        const uint32_t c0 = __float_as_uint(crt::pinned_cos<false>(x)), c1 = __float_as_uint(crt::pinned_cos<true>(x));
        if (s0 != s1) { const unsigned long long k = atomicAdd(&counts[0], 1ull); if (k < 8) samples[k] = bits; }
        if (c0 != c1) { const unsigned long long k = atomicAdd(&counts[1], 1ull); if (k < 8) samples[8 + k] = bits; }
        // that the inputs reach both sides of the range test and both parities: results that are not the out-of-range constants, negative ones
        if (s0 != 0u) atomicAdd(&counts[2], 1ull);
        if ((int32_t)c0 < 0) atomicAdd(&counts[3], 1ull);
    }
}

static uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main() {
    const uint32_t N = 1u << 24;
    std::vector<uint32_t> in;
    in.reserve(N);
    for (uint32_t sign = 0; sign < 2; ++sign) {
        const uint32_t sb = sign << 31;
        in.push_back(sb);                               // +-0
        in.push_back(sb | 0x7f800000u);                 // +-inf
        in.push_back(sb | 0x7fc00000u);                 // NaN
        const uint32_t e9 = f2u(1e9f);
        for (uint32_t k = 0; k < 128; ++k) in.push_back(sb | (e9 - 64u + k));
        for (uint32_t k = 1; k <= 64; ++k) {
            const uint32_t c = f2u((float)((double)k * 3.14159265358979323846));
            for (uint32_t j = 0; j < 4096; ++j) in.push_back(sb | (c - 2048u + j));
            const uint32_t h = f2u((float)(((double)k - 0.5) * 3.14159265358979323846));
            for (uint32_t j = 0; j < 4096; ++j) in.push_back(sb | (h - 2048u + j));
        }
    }
    const uint32_t n_listed = (uint32_t)in.size();
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    for (uint32_t i = 0; in.size() < N; ++i) {
        rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;               // xorshift64
        const uint32_t e = 127u - 30u + (i >> 1) % 61u;                     // biased exponents of 2^-30 .. 2^30 in turn
        in.push_back(((i & 1u) << 31) | (e << 23) | ((uint32_t)(rng >> 20) & 0x007fffffu));
    }
    uint32_t* d_in; unsigned long long* d_counts; uint32_t* d_samples;
    if (hipMalloc(&d_in, N * sizeof(uint32_t)) != hipSuccess || hipMalloc(&d_counts, 4 * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&d_samples, 16 * sizeof(uint32_t)) != hipSuccess) { printf("hip error\n"); return 1; }
    (void)hipMemcpy(d_in, in.data(), N * sizeof(uint32_t), hipMemcpyHostToDevice);
    (void)hipMemset(d_counts, 0, 4 * sizeof(unsigned long long)); (void)hipMemset(d_samples, 0, 16 * sizeof(uint32_t));
    hipLaunchKernelGGL(k_check, dim3(256 * 16), dim3(256), 0, 0, d_in, N, d_counts, d_samples);
    unsigned long long c[4]; uint32_t s[16];
    if (hipMemcpy(c, d_counts, sizeof c, hipMemcpyDeviceToHost) != hipSuccess) { printf("hip error\n"); return 1; }
    (void)hipMemcpy(s, d_samples, sizeof s, hipMemcpyDeviceToHost);
    printf("%u inputs (%u listed, the rest by exponent): pinned_sin differs on %llu, pinned_cos differs on %llu; sine not zero on %llu, cosine negative on %llu\n",
           N, n_listed, c[0], c[1], c[2], c[3]);
    for (int k = 0; k < 2; ++k) { printf("  %s:", k ? "cos" : "sin"); for (int j = 0; j < 8; ++j) if (s[8 * k + j]) printf(" 0x%08x", s[8 * k + j]); printf("\n"); }
    return 0;
}
