// Counter-hash Gaussian shared by random_basis (basis.hip) and matched_noise_edit (matched_noise.hip): entry (j, d)
// of stream `seed` is Box-Muller, in fp64, of two splitmix64 hashes of seed * phi + (j << 32 | d).  A pure function
// of its three arguments (ops.reference.rb_gauss is the same algorithm in numpy).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint64_t rb_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

__device__ __forceinline__ double rb_gauss(uint64_t seed, int j, int d) {
  const uint64_t key = seed * 0x9E3779B97F4A7C15ULL + (((uint64_t)(uint32_t)j << 32) | (uint32_t)d);
  const uint64_t a = rb_mix64(key), b = rb_mix64(key ^ 0xD1B54A32D192ED03ULL);
  const double u1 = ((double)(a >> 11) + 1.0) * 0x1.0p-53;   // (0, 1]
  const double u2 = (double)(b >> 11) * 0x1.0p-53;           // [0, 1)
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// Fixed-order fp64 sum over a 256-thread workgroup (lane butterfly, then the 4 waves in order); red: 4 doubles of LDS
__device__ __forceinline__ double rb_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6;
  __syncthreads();                       // the previous reduction's readers are done with red
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
