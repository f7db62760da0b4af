// Norm-matched random-direction control for the low-rank residual edits.
//
//  matched_noise_edit   per flagged row: the coefficients c_j of lowrank_edit / latent_affine_edit (lowrank_coef.h,
//                       the same device code), the targeted delta  delta = sum_j c_j Dm[idx_j]  in fp32 in slot order
//                       and its norm n = |delta|_2 -- delta itself is never applied.  Instead
//                       h <- bf16(h + n z / |z|_2) with z_d = rb_gauss(seed[row], pos[row], d), the counter-hash
//                       Gaussian of random_basis (rb_gauss.h), then x_next = RMSNorm(h) as lowrank_edit refreshes it.
//                       The row moves exactly as far as the targeted edit would move it, in a direction that depends
//                       only on (seed, absolute position).
//
// A row whose coefficients are all zero, or whose delta is (all-zero decoder rows), keeps h and x_next bit for bit and
// reports norm 0: the control is a no-op exactly where the targeted edit is one.  One workgroup (256 threads) per row,
// D <= 256*8*VPT; every reduction has a fixed order (per-thread chain, lane butterfly, the 4 waves in order), so a
// row's bits depend on its own inputs only, not on the launch or the other rows.
#include "common.h"
#include "api.h"
#include "lowrank_coef.h"
#include "rb_gauss.h"

namespace {

template <typename TT, int VPT, bool AFF>
__global__ void __launch_bounds__(256) matched_noise_edit_kernel(
    uint16_t* __restrict__ h, uint16_t* __restrict__ x_next, const uint8_t* __restrict__ apply,
    const int32_t* __restrict__ idx, const int32_t* __restrict__ cnt, int mmax, const TT* __restrict__ E,
    const TT* __restrict__ Dm, const float* __restrict__ bias, const float* __restrict__ thr,
    const float* __restrict__ pre_bias, float alpha, const uint16_t* __restrict__ w_next, float eps, int D,
    float* __restrict__ coef_out, const float* __restrict__ val, const uint64_t* __restrict__ seeds,
    const int32_t* __restrict__ pos, float* __restrict__ norm_out) {
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  if (norm_out && tid == 0) norm_out[row] = 0.f;   // overwritten below by the one path that edits the row
  if (!apply[row]) return;
  __shared__ float red[16];
  __shared__ double dred[4];
  __shared__ float coef[256];
  const int nvec = D >> 3;
  uint16_t* hr = h + (size_t)row * D;
  const int m = min(cnt[row], min(mmax, 256));
  const int32_t* ir = idx + (size_t)row * mmax;
  lowrank_coefs<TT, AFF>(hr, ir, m, nvec, E, D, bias, thr, pre_bias, alpha,
                         coef_out ? coef_out + (size_t)row * mmax : nullptr,
                         AFF ? val + (size_t)row * mmax : nullptr, coef);
  bool any = false;
  for (int j = 0; j < m; ++j) any |= coef[j] != 0.f;
  if (!any) return;
  // the targeted delta (lowrank_edit's terms in lowrank_edit's order), unrounded and never applied
  float dl[VPT][8];
#pragma unroll
  for (int s = 0; s < VPT; ++s)
#pragma unroll
    for (int q = 0; q < 8; ++q) dl[s][q] = 0.f;
  for (int j = 0; j < m; ++j) {
    const float cj = coef[j];
    if (cj == 0.f) continue;
    const TT* dr = Dm + (size_t)ir[j] * D;
#pragma unroll
    for (int s = 0; s < VPT; ++s) {
      const int i = tid + s * 256;
      if (i < nvec) {
        float df[8];
        load8<TT>(dr + i * 8, df);
#pragma unroll
        for (int q = 0; q < 8; ++q) dl[s][q] += cj * df[q];
      }
    }
  }
  double dd = 0.0;
#pragma unroll
  for (int s = 0; s < VPT; ++s)
#pragma unroll
    for (int q = 0; q < 8; ++q) dd = fma((double)dl[s][q], (double)dl[s][q], dd);
  const float n = (float)sqrt(rb_block_sum(dd, dred));
  if (!(n > 0.f)) return;                          // all-zero decoder rows: nothing to match
  const uint64_t seed = seeds[row];
  const int p = pos[row];
  double z[VPT][8];
  double zz = 0.0;
#pragma unroll
  for (int s = 0; s < VPT; ++s) {
    const int i = tid + s * 256;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      z[s][q] = i < nvec ? rb_gauss(seed, p, i * 8 + q) : 0.0;
      zz = fma(z[s][q], z[s][q], zz);
    }
  }
  const double scale = (double)n / sqrt(rb_block_sum(zz, dred));
  float v[VPT][8];
  float ss = 0.f;
#pragma unroll
  for (int s = 0; s < VPT; ++s) {
    const int i = tid + s * 256;
    if (i < nvec) {
      unpack8(reinterpret_cast<const uint4*>(hr)[i], v[s]);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        v[s][q] = rbf(v[s][q] + (float)(scale * z[s][q]));
        ss += v[s][q] * v[s][q];
      }
      reinterpret_cast<uint4*>(hr)[i] = pack8(v[s]);
    }
  }
  if (norm_out && tid == 0) norm_out[row] = n;
  if (x_next == nullptr) return;
  const float r = rsqrtf(block_sum(ss, red) / (float)D + eps);
#pragma unroll
  for (int s = 0; s < VPT; ++s) {
    const int i = tid + s * 256;
    if (i < nvec) {
      float wf[8], o[8];
      unpack8(reinterpret_cast<const uint4*>(w_next)[i], wf);
#pragma unroll
      for (int q = 0; q < 8; ++q) o[q] = v[s][q] * r * (1.f + wf[q]);
      reinterpret_cast<uint4*>(x_next + (size_t)row * D)[i] = pack8(o);
    }
  }
}

}  // namespace

void tb_matched_noise_edit(uint16_t* h, uint16_t* x_next, const uint8_t* apply, const int32_t* idx,
                           const int32_t* cnt, int mmax, const void* E, const void* Dm, int table_f32,
                           const float* bias, const float* thr, const float* pre_bias, float alpha,
                           const uint16_t* w_next, float eps, int M, int D, float* coef_out, const float* val,
                           const uint64_t* seeds, const int32_t* pos, float* norm_out, hipStream_t st) {
  if (M <= 0) return;
  const int nvec = D >> 3;
#define TB_MN(TT, VPT, AFF)                                                                                        \
  hipLaunchKernelGGL((matched_noise_edit_kernel<TT, VPT, AFF>), dim3(M), dim3(256), 0, st, h, x_next, apply, idx,  \
                     cnt, mmax, (const TT*)E, (const TT*)Dm, bias, thr, pre_bias, alpha, w_next, eps, D, coef_out, \
                     val, seeds, pos, norm_out)
#define TB_MNV(TT, AFF)                                                                                  \
  do {                                                                                                   \
    if (nvec <= 256) TB_MN(TT, 1, AFF); else if (nvec <= 512) TB_MN(TT, 2, AFF); else TB_MN(TT, 4, AFF); \
  } while (0)
  if (val != nullptr) {
    if (table_f32) TB_MNV(float, true); else TB_MNV(uint16_t, true);
  } else {
    if (table_f32) TB_MNV(float, false); else TB_MNV(uint16_t, false);
  }
#undef TB_MNV
#undef TB_MN
}
