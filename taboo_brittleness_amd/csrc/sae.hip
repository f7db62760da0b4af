// SAE and low-rank residual edits.
//
//  gemm_nt_epi      C = A[M,K] . W[N,K]^T on v_mfma_f32_16x16x32_bf16, LDS-tiled
//                   (128x128x64 block tile, 2x2 waves of 64x64, register-staged
//                   double buffer in 2 x (128+128) x 72 bf16 = 72 KB of static LDS --
//                   assumes gfx950's 160 KB LDS, above the 64 KB of older CDNA parts;
//                   K % 64 == 32 is handled by zero-filled chunks, so K % 32 == 0),
//                   with fused epilogues: bf16 store, fp32 store, or Gemma-Scope
//                   JumpReLU (a = pre * [pre > theta], pre = acc + b_enc; strict
//                   '>' as sae_lens).  Used for the dense SAE encode.
//  lowrank_edit     per flagged row:  c_j = f(<h - pre_bias, E_j> + bias_j) * alpha,
//                   h -= sum_j c_j D_j, then x_next = RMSNorm(h) for the next
//                   block.  With E = W_enc^T rows, D = W_dec rows, f = JumpReLU
//                   it is the error-preserving SAE latent ablation (EP:126; only the
//                   m ablated latents are ever encoded); with E = D = U rows,
//                   f = id it is the projection-out x - U U^T x (EP:148).
//  latent_affine_edit  lowrank_edit with a per-row target: h += sum_j (val_j - alpha a_j) D_j, so a latent is
//                   clamped (alpha = 1: held at val_j whether or not it fires) or steered (alpha = 0: val_j added).
//  interchange_edit  lowrank_edit against a donor row: h -= sum_j alpha (a_j(h) - a_j(donor[src[row]])) D_j, so the
//                   selected latents (or subspace coordinates) take the values they have in the donor run.
//  sae_decode_sparse  x_hat = sum_{a_j != 0} a_j W_dec[j] + b_dec (L0 ~ 76 of 16k)
//  sae_splice_edit  reconstruct-mode ablation (EP:126 literal): per flagged row h <- bf16(b_dec + sum over the
//                   active latents, ascending, of s_j a_j W_dec[j]), s_j = 1 - alpha on the ablated ones, then
//                   x_next = RMSNorm(h); activations from a row map (fresh encodes or a per-pair table).
//  flag_compact     [rows] uint8 flags -> row list of static capacity (-1 padded) + inverse map, no host sync.
//  latent_score     score_j = mean_{t in spikes} a_j(t) * max(0, corr_t(a_j, p_secret))
//                   per prompt segment (EP:118-124).
#include "common.h"
#include "api.h"
#include "lowrank_coef.h"

namespace {

constexpr int GBM = 128, GBN = 128, GBK = 64, GLDS = 72;   // padded LDS row (bf16 elements)
constexpr int GCPR = GBK / 8;                               // 16-B chunks per tile row

__device__ __forceinline__ bf16x8 as_bf16x8(const uint4& u) { return __builtin_bit_cast(bf16x8, u); }

template <int EPI>
__global__ void __launch_bounds__(256) gemm_nt_kernel(const uint16_t* __restrict__ A, const uint16_t* __restrict__ W,
                                                      void* __restrict__ C, const float* __restrict__ bias,
                                                      const float* __restrict__ thr, int M, int N, int K, int ldc) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[2][(GBM + GBN) * GLDS];
  // XCD-aware bijective remap of the linear block id (speed only).
  const int nbn = (N + GBN - 1) / GBN, nbm = (M + GBM - 1) / GBM, nwg = nbn * nbm;
  int bid = blockIdx.x;
  {
    const int q = nwg / 8, r = nwg % 8, xcd = bid % 8;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
  }
  const int bn = bid % nbn, bm = bid / nbn;
  const int m0 = bm * GBM, n0 = bn * GBN;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int grp = lane >> 4, col = lane & 15;

  // staging: each operand tile is 128 rows x 8 chunks (16 B) = 1024 chunks, 4 per thread; chunks past K
  // (K % 64 == 32) are zero-filled, so any K % 32 == 0 works
  auto load_tile = [&](int k0, uint4 (&ra)[4], uint4 (&rw)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int id = tid + c * 256, row = id / GCPR, kk = k0 + (id % GCPR) * 8;
      const int ar = m0 + row, wr = n0 + row;
      ra[c] = (ar < M && kk < K) ? *reinterpret_cast<const uint4*>(A + (size_t)ar * K + kk) : make_uint4(0, 0, 0, 0);
      rw[c] = (wr < N && kk < K) ? *reinterpret_cast<const uint4*>(W + (size_t)wr * K + kk) : make_uint4(0, 0, 0, 0);
    }
  };
  auto store_tile = [&](int buf, const uint4 (&ra)[4], const uint4 (&rw)[4]) {
    uint16_t* la = lds[buf];
    uint16_t* lw = lds[buf] + GBM * GLDS;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int id = tid + c * 256, off = (id / GCPR) * GLDS + (id % GCPR) * 8;
      *reinterpret_cast<uint4*>(la + off) = ra[c];
      *reinterpret_cast<uint4*>(lw + off) = rw[c];
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  uint4 ra[4], rw[4];
  load_tile(0, ra, rw);
  store_tile(0, ra, rw);
  __syncthreads();
  const int nk = (K + GBK - 1) / GBK;
  int cur = 0;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) load_tile((kt + 1) * GBK, ra, rw);
    const uint16_t* la = lds[cur];
    const uint16_t* lw = lds[cur] + GBM * GLDS;
#pragma unroll
    for (int ks = 0; ks < GBK / 32; ++ks) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        af[i] = as_bf16x8(*reinterpret_cast<const uint4*>(la + (wm * 64 + i * 16 + col) * GLDS + ks * 32 + grp * 8));
#pragma unroll
      for (int j = 0; j < 4; ++j)
        bfr[j] = as_bf16x8(*reinterpret_cast<const uint4*>(lw + (wn * 64 + j * 16 + col) * GLDS + ks * 32 + grp * 8));
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) store_tile(cur ^ 1, ra, rw);
    __syncthreads();
    cur ^= 1;
  }

  // epilogue: C layout row = 4*grp + r, col = lane&15 inside each 16x16 tile
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + wn * 64 + j * 16 + col;
      if (n >= N) continue;
      float bn_ = 0.f, th = 0.f;
      if (EPI == 2) { bn_ = bias ? bias[n] : 0.f; th = thr ? thr[n] : 0.f; }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm * 64 + i * 16 + 4 * grp + r;
        if (m >= M) continue;
        float v = acc[i][j][r];
        if (EPI == 0) {
          reinterpret_cast<uint16_t*>(C)[(size_t)m * ldc + n] = f2bf(v);
        } else if (EPI == 1) {
          reinterpret_cast<float*>(C)[(size_t)m * ldc + n] = v;
        } else {
          v += bn_;
          reinterpret_cast<float*>(C)[(size_t)m * ldc + n] = (v > th) ? v : 0.f;
        }
      }
    }
}

// ---------------------------------------------------------------- low-rank edit
// (load8 and the coefficient stage live in lowrank_coef.h, shared with matched_noise.hip)
// One workgroup (256 threads) per row; D <= 256*8*VPT.  AFF (latent_affine_edit): the row's coefficient becomes
// alpha * a_j - val[row, j] = -delta_j, so h += sum_j delta_j D_j moves latent j from alpha * a_j to val_j.  The two
// entry points share every other line, so val == 0 gives lowrank_edit's bits.  LR_SWAP (interchange_edit): the
// coefficient is fl32(alpha * a_j(h)) - fl32(alpha * a_j(donor[src[row]])), so the selected coordinates move from the
// row's own values to the donor's; a row whose src is outside the donor table is left alone.  Both products pass
// through LDS before the subtraction, so a row that is its own donor is an exact no-op and the result is
// latent_affine_edit's with val = alpha * a(donor), bit for bit.
constexpr int LR_PLAIN = 0, LR_AFF = 1, LR_SWAP = 2;

template <typename TT, int VPT, int VAR>
__global__ void __launch_bounds__(256) lowrank_edit_kernel(
    uint16_t* __restrict__ h, uint16_t* __restrict__ x_next, const uint8_t* __restrict__ apply,
    const int32_t* __restrict__ idx, const int32_t* __restrict__ cnt, int mmax, const TT* __restrict__ E,
    const TT* __restrict__ Dm, const float* __restrict__ bias, const float* __restrict__ thr,
    const float* __restrict__ pre_bias, float alpha, const uint16_t* __restrict__ w_next, float eps, int D,
    float* __restrict__ coef_out, const float* __restrict__ val, const uint16_t* __restrict__ donor,
    const int32_t* __restrict__ src, int n_donor, float* __restrict__ dcoef_out) {
  const int row = blockIdx.x;
  if (!apply[row]) return;
  const int sr = VAR == LR_SWAP ? src[row] : 0;
  if (VAR == LR_SWAP && (sr < 0 || sr >= n_donor)) return;   // no donor row for this flag: leave the row alone
  __shared__ float red[16];
  __shared__ float coef[256];
  __shared__ float dcoef[VAR == LR_SWAP ? 256 : 1];
  const int nvec = D >> 3;
  const int tid = threadIdx.x;
  uint16_t* hr = h + (size_t)row * D;
  float v[VPT][8];
#pragma unroll
  for (int s = 0; s < VPT; ++s) {
    const int i = tid + s * 256;
    if (i < nvec) unpack8(reinterpret_cast<const uint4*>(hr)[i], v[s]);
    else
#pragma unroll
      for (int j = 0; j < 8; ++j) v[s][j] = 0.f;
  }
  const int m = min(cnt[row], min(mmax, 256));
  const int32_t* ir = idx + (size_t)row * mmax;
  if (VAR == LR_SWAP)
    lowrank_coefs<TT, false>(donor + (size_t)sr * D, ir, m, nvec, E, D, bias, thr, pre_bias, alpha,
                             dcoef_out ? dcoef_out + (size_t)row * mmax : nullptr, nullptr, dcoef);
  lowrank_coefs<TT, VAR == LR_AFF>(hr, ir, m, nvec, E, D, bias, thr, pre_bias, alpha,
                                   coef_out ? coef_out + (size_t)row * mmax : nullptr,
                                   VAR == LR_AFF ? val + (size_t)row * mmax : nullptr, coef);
  if (VAR == LR_SWAP) {
    // both products are fp32 values in LDS here, so the subtraction cannot contract with either of them
    if (tid < m) coef[tid] -= dcoef[tid];
    __syncthreads();
  }
  // an all-zero edit (every ablated latent below its threshold here, or alpha = 0) is an exact no-op: h and
  // x_next stay bit-identical to the unedited forward (no re-rounded h, no re-normalised x)
  bool any = false;
  for (int j = 0; j < m; ++j) any |= coef[j] != 0.f;
  if (!any) return;
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
        for (int q = 0; q < 8; ++q) v[s][q] -= cj * df[q];
      }
    }
  }
  float ss = 0.f;
#pragma unroll
  for (int s = 0; s < VPT; ++s) {
    const int i = tid + s * 256;
    if (i < nvec) {
#pragma unroll
      for (int q = 0; q < 8; ++q) { v[s][q] = rbf(v[s][q]); ss += v[s][q] * v[s][q]; }
      reinterpret_cast<uint4*>(hr)[i] = pack8(v[s]);
    }
  }
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

// ------------------------------------------------------------- sparse decode
template <typename TT>   // decoder table: bf16 (uint16_t) or fp32 (the Gemma Scope dtype, default)
__global__ void __launch_bounds__(256) sae_decode_sparse_kernel(const float* __restrict__ acts,
                                                                const TT* __restrict__ Wdec,
                                                                const float* __restrict__ b_dec,
                                                                uint16_t* __restrict__ out_bf16,
                                                                float* __restrict__ out_f32, int L, int D) {
  __shared__ int act_idx[1024];
  __shared__ float act_val[1024];
  __shared__ int nact;
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* ar = acts + (size_t)row * L;
  if (tid == 0) nact = 0;
  __syncthreads();
  for (int j = tid; j < L; j += blockDim.x) {
    const float a = ar[j];
    if (a != 0.f) {
      const int slot = atomicAdd(&nact, 1);
      if (slot < 1024) { act_idx[slot] = j; act_val[slot] = a; }
    }
  }
  __syncthreads();
  const int nvec = D >> 3;
  if (nact > 1024) {   // dense fallback (only reachable with a badly calibrated SAE)
    for (int c = tid; c < nvec; c += blockDim.x) {
      float o[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) o[q] = b_dec ? b_dec[c * 8 + q] : 0.f;
      for (int j = 0; j < L; ++j) {
        const float a = ar[j];
        if (a == 0.f) continue;
        float wf[8];
        load8<TT>(Wdec + (size_t)j * D + c * 8, wf);
#pragma unroll
        for (int q = 0; q < 8; ++q) o[q] += a * wf[q];
      }
      if (out_bf16) reinterpret_cast<uint4*>(out_bf16 + (size_t)row * D)[c] = pack8(o);
      if (out_f32) {
        float* dst = out_f32 + (size_t)row * D + c * 8;
#pragma unroll
        for (int q = 0; q < 8; ++q) dst[q] = o[q];
      }
    }
    return;
  }
  const int n = nact;
  // deterministic order: sort the (small) active list by index (odd-even transposition)
  for (int phase = 0; phase < n; ++phase) {
    for (int k = tid * 2 + (phase & 1); k + 1 < n; k += 2 * blockDim.x) {
      if (act_idx[k] > act_idx[k + 1]) {
        const int ti = act_idx[k]; act_idx[k] = act_idx[k + 1]; act_idx[k + 1] = ti;
        const float tv = act_val[k]; act_val[k] = act_val[k + 1]; act_val[k + 1] = tv;
      }
    }
    __syncthreads();
  }
  for (int c = tid; c < nvec; c += blockDim.x) {
    float o[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) o[q] = b_dec ? b_dec[c * 8 + q] : 0.f;
    for (int k = 0; k < n; ++k) {
      float wf[8];
      load8<TT>(Wdec + (size_t)act_idx[k] * D + c * 8, wf);
      const float a = act_val[k];
#pragma unroll
      for (int q = 0; q < 8; ++q) o[q] += a * wf[q];
    }
    if (out_bf16) reinterpret_cast<uint4*>(out_bf16 + (size_t)row * D)[c] = pack8(o);
    if (out_f32) {
      float* dst = out_f32 + (size_t)row * D + c * 8;
#pragma unroll
      for (int q = 0; q < 8; ++q) dst[q] = o[q];
    }
  }
}

// --------------------------------------------------------------- splice edit
// Reconstruct-mode ablation: per flagged row  h <- bf16(b_dec + sum_{a_j != 0, ascending j} s_j a_j W_dec[j]),
// s_j = 1 - alpha for j in idx[row, :cnt[row]], else 1; then x_next = RMSNorm(h).  The activations come from
// acts[src_row[row]] (src_row == nullptr: acts[row]), so fresh encodes and rows of a per-pair table share the
// kernel.  One workgroup (256 threads) per row; D <= 256*8*VPT.  The term order is fixed (ascending latent id,
// one fp32 chain per column), so a row's result does not depend on its batch.
constexpr int SPL_CAP = 1024;   // active latents held in LDS; rows above it take the chunked path (same order)

template <typename TT, int VPT>
__global__ void __launch_bounds__(256) sae_splice_edit_kernel(
    uint16_t* __restrict__ h, uint16_t* __restrict__ x_next, const uint8_t* __restrict__ apply,
    const int32_t* __restrict__ src_row, const float* __restrict__ acts, int n_act_rows, int L,
    const int32_t* __restrict__ idx, const int32_t* __restrict__ cnt, int mmax, const TT* __restrict__ Wdec,
    const float* __restrict__ b_dec, float alpha, const uint16_t* __restrict__ w_next, float eps, int D) {
  const int row = blockIdx.x;
  if (!apply[row]) return;
  const int sr = src_row ? src_row[row] : row;
  if (sr < 0 || sr >= n_act_rows) return;          // no activation row for this flag: leave the row alone
  __shared__ int a_idx[SPL_CAP];
  __shared__ float a_val[SPL_CAP];
  __shared__ int s_idx[SPL_CAP];
  __shared__ float s_val[SPL_CAP];
  __shared__ int abl[256];
  __shared__ float red[16];
  __shared__ int nact;
  const int tid = threadIdx.x;
  const int nvec = D >> 3;
  const float* ar = acts + (size_t)sr * L;
  const int m = max(0, min(cnt[row], min(mmax, 256)));
  const float keep = 1.f - alpha;
  if (tid == 0) nact = 0;
  if (tid < m) abl[tid] = idx[(size_t)row * mmax + tid];
  __syncthreads();
  for (int j = tid; j < L; j += 256) {
    const float a = ar[j];
    if (a != 0.f) {
      const int slot = atomicAdd(&nact, 1);
      if (slot < SPL_CAP) { a_idx[slot] = j; a_val[slot] = a; }
    }
  }
  __syncthreads();
  const int n = nact;
  float v[VPT][8];
#pragma unroll
  for (int s = 0; s < VPT; ++s) {
    const int i = tid + s * 256;
#pragma unroll
    for (int q = 0; q < 8; ++q) v[s][q] = (b_dec && i < nvec) ? b_dec[i * 8 + q] : 0.f;
  }
  if (n <= SPL_CAP) {
    // rank sort by latent id (ids are unique) with the row's scale applied: s_val[k] = s_j * a_j
    for (int k = tid; k < n; k += 256) {
      const int j = a_idx[k];
      int rank = 0;
      for (int t = 0; t < n; ++t) rank += a_idx[t] < j;
      bool ab = false;
      for (int t = 0; t < m; ++t) ab |= abl[t] == j;
      s_idx[rank] = j;
      s_val[rank] = ab ? keep * a_val[k] : a_val[k];
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
      const float c = s_val[k];
      const TT* dr = Wdec + (size_t)s_idx[k] * D;
#pragma unroll
      for (int s = 0; s < VPT; ++s) {
        const int i = tid + s * 256;
        if (i < nvec) {
          float df[8];
          load8<TT>(dr + i * 8, df);
#pragma unroll
          for (int q = 0; q < 8; ++q) v[s][q] = fmaf(c, df[q], v[s][q]);
        }
      }
    }
  } else {
    // more active latents than the LDS list holds (a badly calibrated SAE): chunks of SPL_CAP consecutive latents,
    // each scaled in parallel and then accumulated in ascending id -- the same terms in the same order
    for (int base = 0; base < L; base += SPL_CAP) {
      __syncthreads();
      for (int k = tid; k < SPL_CAP; k += 256) {
        const int j = base + k;
        const float a = j < L ? ar[j] : 0.f;
        float c = a;
        if (a != 0.f) {
          bool ab = false;
          for (int t = 0; t < m; ++t) ab |= abl[t] == j;
          if (ab) c = keep * a;
        }
        s_idx[k] = a != 0.f;
        s_val[k] = c;
      }
      __syncthreads();
      for (int k = 0; k < SPL_CAP; ++k) {
        if (!s_idx[k]) continue;
        const float c = s_val[k];
        const TT* dr = Wdec + (size_t)(base + k) * D;
#pragma unroll
        for (int s = 0; s < VPT; ++s) {
          const int i = tid + s * 256;
          if (i < nvec) {
            float df[8];
            load8<TT>(dr + i * 8, df);
#pragma unroll
            for (int q = 0; q < 8; ++q) v[s][q] = fmaf(c, df[q], v[s][q]);
          }
        }
      }
    }
  }
  uint16_t* hr = h + (size_t)row * D;
  float ss = 0.f;
#pragma unroll
  for (int s = 0; s < VPT; ++s) {
    const int i = tid + s * 256;
    if (i < nvec) {
#pragma unroll
      for (int q = 0; q < 8; ++q) { v[s][q] = rbf(v[s][q]); ss += v[s][q] * v[s][q]; }
      reinterpret_cast<uint4*>(hr)[i] = pack8(v[s]);
    }
  }
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

// -------------------------------------------------------------- flag compact
// rows[0 .. count) = the indices i < n with flags[i] != 0 in ascending order, rows[count .. cap) = -1; inv[i]
// (optional) = the list position of row i, -1 if unflagged.  Flags past the capacity are dropped (inv = -1), never
// written out of range.  One workgroup of 1024 threads walks the flags in chunks with a running offset.
__global__ void __launch_bounds__(1024) flag_compact_kernel(const uint8_t* __restrict__ flags, int n,
                                                            int32_t* __restrict__ rows, int cap,
                                                            int32_t* __restrict__ inv) {
  __shared__ int wsum[16];
  __shared__ int run;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid == 0) run = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int i = base + tid;
    const bool f = i < n && flags[i] != 0;
    const unsigned long long bal = __ballot(f);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wid] = __popcll(bal);
    __syncthreads();
    int off = run;
    for (int w = 0; w < wid; ++w) off += wsum[w];
    const int p = off + before;
    if (f && p < cap) rows[p] = i;
    if (inv != nullptr && i < n) inv[i] = (f && p < cap) ? p : -1;
    __syncthreads();
    if (tid == 0) {
      int t = run;
      for (int w = 0; w < 16; ++w) t += wsum[w];
      run = t;
    }
    __syncthreads();
  }
  const int total = min(run, cap);
  for (int p = total + tid; p < cap; p += 1024) rows[p] = -1;
}

// ------------------------------------------------------------- latent score
// grid (ceil(L/256), G): segment g covers rows seg[g] .. seg[g+1]-1.
__global__ void __launch_bounds__(256) latent_score_kernel(const float* __restrict__ acts,
                                                           const float* __restrict__ p,
                                                           const uint8_t* __restrict__ spike,
                                                           const int32_t* __restrict__ seg, float* __restrict__ out,
                                                           float* __restrict__ spike_mean_out,
                                                           float* __restrict__ corr_out, int L) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int g = blockIdx.y;
  if (j >= L) return;
  const int r0 = seg[g], r1 = seg[g + 1];
  const int n = r1 - r0;
  // two passes in fp64 (means, then centred sums): the one-pass saa - sa^2/n form cancels
  // catastrophically for offset, low-variance latents (a ~ 40 +- 0.01) and could push a noisy
  // correlation into the targeted set.  n is a prompt's length, so the second read hits L2.
  double sa = 0.0, sp = 0.0, ssp = 0.0;
  int nsp = 0;
  for (int r = r0; r < r1; ++r) {
    const double a = acts[(size_t)r * L + j];
    sa += a; sp += (double)p[r];
    if (spike[r]) { ssp += a; ++nsp; }
  }
  float corr = 0.f;
  if (n > 1) {
    const double ma = sa / n, mp = sp / n;
    double va = 0.0, vp = 0.0, cov = 0.0;
    for (int r = r0; r < r1; ++r) {
      const double ac = (double)acts[(size_t)r * L + j] - ma, pc = (double)p[r] - mp;
      va += ac * ac; vp += pc * pc; cov += ac * pc;
    }
    if (va > 1e-12 && vp > 1e-20) corr = (float)(cov / sqrt(va * vp));
  }
  const float sm = nsp ? (float)(ssp / nsp) : 0.f;
  out[(size_t)g * L + j] = sm * fmaxf(corr, 0.f);
  if (spike_mean_out) spike_mean_out[(size_t)g * L + j] = sm;
  if (corr_out) corr_out[(size_t)g * L + j] = corr;
}

}  // namespace

void tb_gemm_nt(const uint16_t* A, const uint16_t* W, void* C, const float* bias, const float* thr, int M, int N,
                int K, int ldc, int epi, hipStream_t st) {
  if (M <= 0 || N <= 0) return;
  const int nwg = ((N + GBN - 1) / GBN) * ((M + GBM - 1) / GBM);
  if (epi == 0) hipLaunchKernelGGL(gemm_nt_kernel<0>, dim3(nwg), dim3(256), 0, st, A, W, C, bias, thr, M, N, K, ldc);
  else if (epi == 1) hipLaunchKernelGGL(gemm_nt_kernel<1>, dim3(nwg), dim3(256), 0, st, A, W, C, bias, thr, M, N, K, ldc);
  else hipLaunchKernelGGL(gemm_nt_kernel<2>, dim3(nwg), dim3(256), 0, st, A, W, C, bias, thr, M, N, K, ldc);
}

// the lowrank_edit_kernel family: val -> LR_AFF, donor -> LR_SWAP, neither -> LR_PLAIN
static void launch_lowrank(uint16_t* h, uint16_t* x_next, const uint8_t* apply, const int32_t* idx,
                           const int32_t* cnt, int mmax, const void* E, const void* Dm, int table_f32,
                           const float* bias, const float* thr, const float* pre_bias, float alpha,
                           const uint16_t* w_next, float eps, int M, int D, float* coef_out, hipStream_t st,
                           const float* val, const uint16_t* donor, const int32_t* src, int n_donor,
                           float* dcoef_out) {
  if (M <= 0) return;
  const int nvec = D >> 3;
#define TB_LR(TT, VPT, VAR)                                                                                      \
  hipLaunchKernelGGL((lowrank_edit_kernel<TT, VPT, VAR>), dim3(M), dim3(256), 0, st, h, x_next, apply, idx, cnt, \
                     mmax, (const TT*)E, (const TT*)Dm, bias, thr, pre_bias, alpha, w_next, eps, D, coef_out, val, \
                     donor, src, n_donor, dcoef_out)
#define TB_LRV(TT, VAR)                                                                                  \
  do {                                                                                                   \
    if (nvec <= 256) TB_LR(TT, 1, VAR); else if (nvec <= 512) TB_LR(TT, 2, VAR); else TB_LR(TT, 4, VAR); \
  } while (0)
  if (donor != nullptr) {
    if (table_f32) TB_LRV(float, LR_SWAP); else TB_LRV(uint16_t, LR_SWAP);
  } else if (val != nullptr) {
    if (table_f32) TB_LRV(float, LR_AFF); else TB_LRV(uint16_t, LR_AFF);
  } else {
    if (table_f32) TB_LRV(float, LR_PLAIN); else TB_LRV(uint16_t, LR_PLAIN);
  }
#undef TB_LRV
#undef TB_LR
}

void tb_lowrank_edit(uint16_t* h, uint16_t* x_next, const uint8_t* apply, const int32_t* idx, const int32_t* cnt,
                     int mmax, const void* E, const void* Dm, int table_f32, const float* bias, const float* thr,
                     const float* pre_bias, float alpha, const uint16_t* w_next, float eps, int M, int D,
                     float* coef_out, hipStream_t st, const float* val) {
  launch_lowrank(h, x_next, apply, idx, cnt, mmax, E, Dm, table_f32, bias, thr, pre_bias, alpha, w_next, eps, M, D,
                 coef_out, st, val, nullptr, nullptr, 0, nullptr);
}

void tb_interchange_edit(uint16_t* h, uint16_t* x_next, const uint8_t* apply, const int32_t* idx, const int32_t* cnt,
                         int mmax, const void* E, const void* Dm, int table_f32, const float* bias, const float* thr,
                         const float* pre_bias, float alpha, const uint16_t* w_next, float eps, int M, int D,
                         float* coef_out, const uint16_t* donor, const int32_t* src, int n_donor, float* dcoef_out,
                         hipStream_t st) {
  if (donor == nullptr || src == nullptr || n_donor <= 0) return;   // no donor table: every row is left alone
  launch_lowrank(h, x_next, apply, idx, cnt, mmax, E, Dm, table_f32, bias, thr, pre_bias, alpha, w_next, eps, M, D,
                 coef_out, st, nullptr, donor, src, n_donor, dcoef_out);
}

void tb_sae_decode_sparse(const float* acts, const void* Wdec, int table_f32, const float* b_dec, uint16_t* out_bf16,
                          float* out_f32, int M, int L, int D, hipStream_t st) {
  if (M <= 0) return;
  if (table_f32)
    hipLaunchKernelGGL(sae_decode_sparse_kernel<float>, dim3(M), dim3(256), 0, st, acts,
                       reinterpret_cast<const float*>(Wdec), b_dec, out_bf16, out_f32, L, D);
  else
    hipLaunchKernelGGL(sae_decode_sparse_kernel<uint16_t>, dim3(M), dim3(256), 0, st, acts,
                       reinterpret_cast<const uint16_t*>(Wdec), b_dec, out_bf16, out_f32, L, D);
}

void tb_sae_splice_edit(uint16_t* h, uint16_t* x_next, const uint8_t* apply, const int32_t* src_row,
                        const float* acts, int n_act_rows, int L, const int32_t* idx, const int32_t* cnt, int mmax,
                        const void* Wdec, int table_f32, const float* b_dec, float alpha, const uint16_t* w_next,
                        float eps, int M, int D, hipStream_t st) {
  if (M <= 0) return;
  const int nvec = D >> 3;
#define TB_SPL(TT, VPT)                                                                                            \
  hipLaunchKernelGGL((sae_splice_edit_kernel<TT, VPT>), dim3(M), dim3(256), 0, st, h, x_next, apply, src_row, acts, \
                     n_act_rows, L, idx, cnt, mmax, (const TT*)Wdec, b_dec, alpha, w_next, eps, D)
  if (table_f32) {
    if (nvec <= 256) TB_SPL(float, 1); else if (nvec <= 512) TB_SPL(float, 2); else TB_SPL(float, 4);
  } else {
    if (nvec <= 256) TB_SPL(uint16_t, 1); else if (nvec <= 512) TB_SPL(uint16_t, 2); else TB_SPL(uint16_t, 4);
  }
#undef TB_SPL
}

void tb_flag_compact(const uint8_t* flags, int n, int32_t* rows, int cap, int32_t* inv, hipStream_t st) {
  if (cap <= 0 && (inv == nullptr || n <= 0)) return;
  hipLaunchKernelGGL(flag_compact_kernel, dim3(1), dim3(1024), 0, st, flags, n, rows, cap, inv);
}

void tb_latent_score(const float* acts, const float* p, const uint8_t* spike, const int32_t* seg, float* out,
                     float* spike_mean, float* corr, int G, int L, hipStream_t st) {
  if (G <= 0) return;
  dim3 grid((L + 255) / 256, G);
  hipLaunchKernelGGL(latent_score_kernel, grid, dim3(256), 0, st, acts, p, spike, seg, out, spike_mean, corr, L);
}
