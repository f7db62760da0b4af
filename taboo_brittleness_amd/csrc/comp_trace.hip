// Component trace: segment-wise dot products of selected rows against a per-pair table, over the row's own RMS.
//
//  seg_dots   out[i, t, s] = ( sum_{k in segment s} X[rows[i], k] * W[blk[i], t, k] ) / rho_i
//             rho_i = sqrt(|R[rows[i]]|^2 / Dn + eps)   (1 without R),   rms[i] = rho_i
//             for X [M, K] bf16, a table W [U, T, K] fp32, the selected rows rows [Ms] and their table blocks
//             blk [Ms] (int32), S segments of K / S columns each, R [M, Dn] bf16.  rows[i] outside [0, M) or blk[i]
//             outside [0, U) writes +0.0 in all T * S columns and rms[i] = 0.0, and reads nothing.
//
// With X the heads' outputs before o_proj and W the lens direction pulled back through o_proj, segment s is head s's
// direct contribution to the lens logit; with S = 1 it is a plain dot product (MLP output, residual).
//
// One wave takes one selected row; a workgroup is four independent waves (no LDS, no barrier).  A segment is
// gs = K / (8 S) 8-column groups and is reduced by a team of Wd = min(64, 2^ceil(log2 gs)) lanes, so a wave finishes
// 64 / Wd segments per pass: lane j of a team owns groups j, j + Wd, ... of its segment in ascending order (one group
// when Wd < 64), each group is eight fp32 FMAs in column order into one accumulator per t, and the team's sums go
// through the xor butterfly from Wd / 2 down to 1.  |R|^2 runs in the same style over the whole wave (lens_track's
// chain).  The quotient and the root are fp64 with one fp32 store.  The order is a function of (K, S) and Dn alone,
// so a row's bits do not depend on Ms, on its place in the launch or on its neighbours' rows / blk.
#include "common.h"
#include "api.h"

namespace {

constexpr int SD_THREADS = 256, SD_WAVES = SD_THREADS / 64;

__device__ __forceinline__ float sd_dot8(const float* a, const float4& bl, const float4& bh, float acc) {
  acc = fmaf(a[0], bl.x, acc); acc = fmaf(a[1], bl.y, acc); acc = fmaf(a[2], bl.z, acc); acc = fmaf(a[3], bl.w, acc);
  acc = fmaf(a[4], bh.x, acc); acc = fmaf(a[5], bh.y, acc); acc = fmaf(a[6], bh.z, acc); acc = fmaf(a[7], bh.w, acc);
  return acc;
}

// sum over the aligned team of Wd lanes (Wd a power of two, wave-uniform): every lane of the team holds it
__device__ __forceinline__ float sd_team_sum(float v, int Wd) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float other = __shfl_xor(v, o, 64);
    if (o < Wd) v += other;
  }
  return v;
}

template <int T>
__global__ void __launch_bounds__(SD_THREADS) seg_dots_kernel(
    const uint16_t* __restrict__ X, const float* __restrict__ W, const int32_t* __restrict__ rows,
    const int32_t* __restrict__ blk, const uint16_t* __restrict__ R, float* __restrict__ out,
    float* __restrict__ rms, int M, int U, int Ms, int K, int S, int Dn, int Wd, double eps) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * SD_WAVES + (threadIdx.x >> 6);      // wave-uniform
  if (i >= Ms) return;
  float* __restrict__ o = out + (size_t)i * T * S;
  const int r = rows[i], u = blk[i];
  if (r < 0 || r >= M || u < 0 || u >= U) {
    for (int c = lane; c < T * S; c += 64) o[c] = 0.f;
    if (lane == 0) rms[i] = 0.f;
    return;
  }
  double rho = 1.0;
  if (R != nullptr) {
    const uint16_t* __restrict__ rr = R + (size_t)r * Dn;
    float xx = 0.f;
    for (int c = lane; c < (Dn >> 3); c += 64) {
      float f[8];
      unpack8(*reinterpret_cast<const uint4*>(rr + c * 8), f);
#pragma unroll
      for (int k = 0; k < 8; ++k) xx = fmaf(f[k], f[k], xx);
    }
    xx = wave_sum(xx);
    rho = sqrt((double)xx / (double)Dn + eps);
  }
  if (lane == 0) rms[i] = (float)rho;

  const uint16_t* __restrict__ xr = X + (size_t)r * K;
  const float* __restrict__ wb = W + (size_t)u * T * K;
  const int gs = (K >> 3) / S;                 // groups per segment
  const int per = 64 / Wd;                     // segments per pass
  const int team = lane / Wd, j = lane - team * Wd;
  for (int s0 = 0; s0 < S; s0 += per) {
    const int s = s0 + team;
    float acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = 0.f;
    if (s < S) {
      for (int g = j; g < gs; g += Wd) {
        const int c = (s * gs + g) * 8;          // < K
        float f[8];
        unpack8(*reinterpret_cast<const uint4*>(xr + c), f);
#pragma unroll
        for (int t = 0; t < T; ++t) {
          const float4* p = reinterpret_cast<const float4*>(wb + (size_t)t * K + c);
          const float4 wl = p[0], wh = p[1];
          acc[t] = sd_dot8(f, wl, wh, acc[t]);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const float d = sd_team_sum(acc[t], Wd);
      if (j == 0 && s < S) o[t * S + s] = (float)((double)d / rho);
    }
  }
}

}  // namespace

int tb_seg_dots(const uint16_t* X, const float* W, const int32_t* rows, const int32_t* blk, const uint16_t* R,
                float* out, float* rms, int M, int U, int Ms, int T, int K, int S, int Dn, double eps,
                hipStream_t st) {
  if (T < 1 || T > 4 || S < 1 || S > 64 || K < 8 || (K & 7) || K > 4096 || (K % S) || ((K / S) & 7)) return 3;
  if (R != nullptr && (Dn < 8 || (Dn & 7) || Dn > 4096)) return 3;
  if (M < 0 || U < 0 || Ms < 0) return 3;
  if (Ms == 0) return 0;
  const int gs = (K >> 3) / S;
  int Wd = 1;
  while (Wd < gs && Wd < 64) Wd <<= 1;
  const dim3 grid((Ms + SD_WAVES - 1) / SD_WAVES), block(SD_THREADS);
#define TB_SD(TT)                                                                                                  \
  case TT:                                                                                                         \
    hipLaunchKernelGGL((seg_dots_kernel<TT>), grid, block, 0, st, X, W, rows, blk, R, out, rms, M, U, Ms, K, S, Dn, \
                       Wd, eps);                                                                                   \
    break
  switch (T) {
    TB_SD(1); TB_SD(2); TB_SD(3); TB_SD(4);
  }
#undef TB_SD
  return 0;
}
