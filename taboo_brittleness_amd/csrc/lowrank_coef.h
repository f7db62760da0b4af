// The coefficient stage shared by the per-row low-rank edits (lowrank_edit / latent_affine_edit in sae.hip,
// matched_noise_edit in matched_noise.hip): one definition, so the kernels agree bit for bit on a_j, on alpha * a_j
// (- val_j) and therefore on which rows are exact no-ops.
#pragma once
#include "common.h"

template <typename TT>
__device__ __forceinline__ void load8(const TT* p, float* f);
template <>
__device__ __forceinline__ void load8<uint16_t>(const uint16_t* p, float* f) {
  unpack8(*reinterpret_cast<const uint4*>(p), f);
}
template <>
__device__ __forceinline__ void load8<float>(const float* p, float* f) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

// One workgroup of 256 threads on row hr [D = 8 nvec]: coef[j] = alpha * a_j, a_j = f(<h - pre_bias, E[ir[j]]> +
// bias) with f = JumpReLU (thr) or id, for j < m <= 256; AFF: coef[j] -= val_row[j].  coef_row (optional) receives
// a_j.  Ends with a barrier: every thread may read coef[0 .. m) on return.
template <typename TT, bool AFF>
__device__ __forceinline__ void lowrank_coefs(const uint16_t* hr, const int32_t* ir, int m, int nvec, const TT* E,
                                              int D, const float* bias, const float* thr, const float* pre_bias,
                                              float alpha, float* coef_row, const float* val_row, float* coef) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  // waves split the m directions, lanes split D
  for (int j = wid; j < m; j += 4) {
    const int e = ir[j];
    const TT* er = E + (size_t)e * D;
    float part = 0.f;
    for (int c = lane; c < nvec; c += 64) {
      float ef[8], hf[8];
      load8<TT>(er + c * 8, ef);
      unpack8(reinterpret_cast<const uint4*>(hr)[c], hf);
      if (pre_bias) {
#pragma unroll
        for (int q = 0; q < 8; ++q) hf[q] -= pre_bias[c * 8 + q];
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) part += hf[q] * ef[q];
    }
    part = wave_sum(part);
    if (lane == 0) {
      float pre = part + (bias ? bias[e] : 0.f);
      float a = pre;
      if (thr) a = (pre > thr[e]) ? pre : 0.f;
      coef[j] = alpha * a;
      if (coef_row) coef_row[j] = a;
    }
  }
  __syncthreads();
  if (AFF) {
    // alpha * a_j went through LDS as an fp32 value, so the subtraction cannot contract with the product
    if (tid < m) coef[tid] -= val_row[tid];
    __syncthreads();
  }
}
