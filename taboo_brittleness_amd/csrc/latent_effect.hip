// Causal latent scores at the spike rows (the counterpart of latent_score's correlational rule).
//
//  latent_effect   per spike row t and latent j with a = acts[t, j] > 0, c = alpha * a, d = W_dec[j]:
//                    mode 0 (effect_lens)  eff = f(z(x)) - f(z(x - c d)),  z(y) = (y . v) / sqrt(|y|^2 / D + eps),
//                                          f = the softcap cap * tanh(. / cap) (cap <= 0: identity): the exact
//                                          change of the secret token's logit-lens logit when latent j alone is
//                                          ablated (v = lm_head[s] * (1 + norm_f)).  Closed form in three dot
//                                          products: (x - c d) . v = xu - c q, |x - c d|^2 = xx - 2 c p + c^2 s
//                                          with p = x . d, q = v . d, s = d . d.
//                    mode 1 (attr_model)   eff = c q: first-order attribution, v = the row's gradient.
//                  a <= 0: eff = 0 exactly and the decoder row is never read.
//                  score[g, j] = mean over the rows of segment g of eff[., j] (ascending rows, fp64).
//
// One workgroup (256 threads) per spike row: x and v are staged in LDS as fp32, the row's active latent ids are
// compacted in ascending order into a bounded list that is flushed whenever it could overflow (any active count up
// to L works), and each wave takes one listed latent at a time with 16-byte loads of its decoder row.  The D-long
// dot products accumulate in fp32 in a fixed order per lane and a fixed-order wave reduction; the scalar tail is
// fp64 (the two quotients differ in the fourth or fifth digit).  A row's result depends on that row alone, and a
// segment's score on its own rows alone, so both are bit-identical in any launch.
#include "common.h"
#include "api.h"

namespace {

constexpr int LE_THREADS = 256, LE_WAVES = LE_THREADS / 64;
constexpr int LE_CAP = 512;       // listed active latents; flushed once fewer than LE_THREADS slots are free
constexpr int LE_DMAX = 4096;

template <typename TT>
__device__ __forceinline__ void le_load8(const TT* p, float4& lo, float4& hi);
template <>
__device__ __forceinline__ void le_load8<float>(const float* p, float4& lo, float4& hi) {
  lo = reinterpret_cast<const float4*>(p)[0];
  hi = reinterpret_cast<const float4*>(p)[1];
}
template <>
__device__ __forceinline__ void le_load8<uint16_t>(const uint16_t* p, float4& lo, float4& hi) {
  float f[8];
  unpack8(*reinterpret_cast<const uint4*>(p), f);
  lo = make_float4(f[0], f[1], f[2], f[3]);
  hi = make_float4(f[4], f[5], f[6], f[7]);
}

__device__ __forceinline__ float dot4(const float4& a, const float4& b, float acc) {
  acc = fmaf(a.x, b.x, acc); acc = fmaf(a.y, b.y, acc);
  acc = fmaf(a.z, b.z, acc); acc = fmaf(a.w, b.w, acc);
  return acc;
}

__device__ __forceinline__ double softcap64(double z, double cap) { return cap > 0.0 ? cap * tanh(z / cap) : z; }

// LDS layout of a staged row: 16-byte chunk c of the 8-element group g = c / 2 lives in plane (c & 1) at float
// offset plane * (D / 2) + g * 4, so the two ds_read_b128 of a lane are each lane-contiguous (no bank conflicts).
template <typename TT, int MODE>
__global__ void __launch_bounds__(LE_THREADS) latent_effect_kernel(
    const float* __restrict__ acts, const uint16_t* __restrict__ X, const float* __restrict__ V, int v_per_row,
    const TT* __restrict__ Wdec, float* __restrict__ eff, int L, int D, double alpha, double eps, double cap) {
  __shared__ __attribute__((aligned(16))) float xs[LE_DMAX];
  __shared__ __attribute__((aligned(16))) float vs[LE_DMAX];
  __shared__ int ids[LE_CAP];
  __shared__ float av[LE_CAP];
  __shared__ int wsum[LE_WAVES];
  __shared__ float red[16];
  __shared__ double rowc[3];        // xu, xx, f(z(x))
  const int row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nvec = D >> 3, half = D >> 1;
  const uint16_t* xr = X + (size_t)row * D;
  const float* vr = V + (v_per_row ? (size_t)row * D : 0);
  const float* ar = acts + (size_t)row * L;
  float* er = eff + (size_t)row * L;

  float xu = 0.f, xx = 0.f;
  for (int c = tid; c < nvec; c += LE_THREADS) {
    float4 xl, xh, vl, vh;
    le_load8<uint16_t>(xr + c * 8, xl, xh);
    le_load8<float>(vr + c * 8, vl, vh);
    *reinterpret_cast<float4*>(xs + c * 4) = xl;
    *reinterpret_cast<float4*>(xs + half + c * 4) = xh;
    *reinterpret_cast<float4*>(vs + c * 4) = vl;
    *reinterpret_cast<float4*>(vs + half + c * 4) = vh;
    if (MODE == 0) {
      xu = dot4(xl, vl, xu); xu = dot4(xh, vh, xu);
      xx = dot4(xl, xl, xx); xx = dot4(xh, xh, xx);
    }
  }
  if (MODE == 0) {
    xu = block_sum(xu, red);
    xx = block_sum(xx, red);
    if (tid == 0) {
      rowc[0] = (double)xu;
      rowc[1] = (double)xx;
      rowc[2] = softcap64((double)xu / sqrt((double)xx / (double)D + eps), cap);
    }
  }
  __syncthreads();

  int n = 0;                        // listed latents (uniform across the workgroup)
  for (int base = 0; base < L; base += LE_THREADS) {
    const int j = base + tid;
    const float a = j < L ? ar[j] : 0.f;
    const bool f = a > 0.f;
    if (j < L && !f) er[j] = 0.f;
    const unsigned long long bal = __ballot(f);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wid] = __popcll(bal);
    __syncthreads();
    int off = n, tot = 0;
#pragma unroll
    for (int w = 0; w < LE_WAVES; ++w) {
      if (w < wid) off += wsum[w];
      tot += wsum[w];
    }
    if (f) { ids[off + before] = j; av[off + before] = a; }
    n += tot;
    __syncthreads();
    if (n <= LE_CAP - LE_THREADS && base + LE_THREADS < L) continue;
    // flush: one wave per listed latent
    for (int k = wid; k < n; k += LE_WAVES) {
      const int jj = ids[k];
      const TT* dr = Wdec + (size_t)jj * D;
      float p = 0.f, q = 0.f, s = 0.f;
#pragma unroll 2
      for (int c = lane; c < nvec; c += 64) {
        float4 dl, dh;
        le_load8<TT>(dr + c * 8, dl, dh);
        const float4 vl = *reinterpret_cast<const float4*>(vs + c * 4);
        const float4 vh = *reinterpret_cast<const float4*>(vs + half + c * 4);
        q = dot4(vl, dl, q); q = dot4(vh, dh, q);
        if (MODE == 0) {
          const float4 xl = *reinterpret_cast<const float4*>(xs + c * 4);
          const float4 xh = *reinterpret_cast<const float4*>(xs + half + c * 4);
          p = dot4(xl, dl, p); p = dot4(xh, dh, p);
          s = dot4(dl, dl, s); s = dot4(dh, dh, s);
        }
      }
      q = wave_sum(q);
      if (MODE == 0) { p = wave_sum(p); s = wave_sum(s); }
      if (lane == 0) {
        const double cj = alpha * (double)av[k];
        double e;
        if (MODE == 0) {
          const double num = rowc[0] - cj * (double)q;
          const double ss = fmax(rowc[1] - 2.0 * cj * (double)p + cj * cj * (double)s, 0.0);
          e = rowc[2] - softcap64(num / sqrt(ss / (double)D + eps), cap);
        } else {
          e = cj * (double)q;
        }
        er[jj] = (float)e;
      }
    }
    n = 0;
    __syncthreads();
  }
}

// grid (ceil(L/256), G): score[g, j] = mean of eff[seg[g] .. seg[g+1]-1, j], ascending rows, fp64; empty: 0.
__global__ void __launch_bounds__(256) latent_effect_mean_kernel(const float* __restrict__ eff,
                                                                 const int32_t* __restrict__ seg,
                                                                 float* __restrict__ score, int R, int L) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int g = blockIdx.y;
  if (j >= L) return;
  const int r0 = max(seg[g], 0), r1 = min(seg[g + 1], R);   // a malformed seg never reads outside eff
  double s = 0.0;
  for (int r = r0; r < r1; ++r) s += (double)eff[(size_t)r * L + j];
  score[(size_t)g * L + j] = r1 > r0 ? (float)(s / (double)(r1 - r0)) : 0.f;
}

}  // namespace

void tb_latent_effect(const float* acts, const uint16_t* X, const float* V, int v_per_row, const void* Wdec,
                      int table_f32, const int32_t* seg, float* score, float* eff, int R, int G, int L, int D,
                      double alpha, double eps, double cap, int mode, hipStream_t st) {
#define TB_LE(TT, MODE)                                                                                            \
  hipLaunchKernelGGL((latent_effect_kernel<TT, MODE>), dim3(R), dim3(LE_THREADS), 0, st, acts, X, V, v_per_row, \
                     (const TT*)Wdec, eff, L, D, alpha, eps, cap)
  if (R > 0 && L > 0) {
    if (table_f32) { if (mode == 0) TB_LE(float, 0); else TB_LE(float, 1); }
    else { if (mode == 0) TB_LE(uint16_t, 0); else TB_LE(uint16_t, 1); }
  }
#undef TB_LE
  if (G > 0 && L > 0 && score != nullptr) {
    dim3 grid((L + 255) / 256, G);
    hipLaunchKernelGGL(latent_effect_mean_kernel, grid, dim3(256), 0, st, eff, seg, score, R, L);
  }
}
