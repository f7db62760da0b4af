// Layer trace: the tracked tokens' capped logit-lens logits of residual rows, without the vocabulary GEMM.
//
//  lens_track   out[r, t] = f( (h_r . V[vrow[r], t]) / sqrt(|h_r|^2 / D + eps) ),  f = cap * tanh(. / cap)
//               (cap <= 0: identity), for h [M, D] bf16, a table V [U, T, D] fp32 (v = lm_head[id] * (1 + norm_f),
//               latent_effect's mode-0 readout) and a device row map vrow [M].  vrow[r] outside [0, U) writes 0.0 in
//               all T columns and reads no table row.
//
// One workgroup (256 threads) takes LT_ROWS = 16 consecutive rows, four per wave.  Rows arrive ordered by cell, so
// the rows of a workgroup nearly always share one table block: the block of the workgroup's first row is staged in
// LDS one 512-column chunk at a time (T * 2 KB), and a wave whose four rows all use it reads each 16-byte piece of
// the table once from LDS for its four rows.  A wave with any other row (another block, a skipped row, the ragged end
// of the launch) takes its rows one at a time against the table in global memory.  Both paths run the same
// arithmetic: lane l owns the 8-column groups l, l + 64, ... of a row in ascending order, each group is eight fp32
// FMAs in column order into one accumulator per (row, t) and one for |h|^2, the 64 lane sums go through the
// fixed-order wave butterfly, and the quotient and the cap are fp64.  A row's bits therefore depend on that row and
// its table block alone: not on M, on its place in the launch or on its neighbours' vrow.
#include "common.h"
#include "api.h"

namespace {

constexpr int LT_THREADS = 256, LT_WAVES = LT_THREADS / 64, LT_RPW = 4, LT_ROWS = LT_WAVES * LT_RPW;
constexpr int LT_CHUNK = 64;      // 8-column groups per staged chunk: one per lane

__device__ __forceinline__ float lt_dot8(const float* a, const float4& bl, const float4& bh, float acc) {
  acc = fmaf(a[0], bl.x, acc); acc = fmaf(a[1], bl.y, acc); acc = fmaf(a[2], bl.z, acc); acc = fmaf(a[3], bl.w, acc);
  acc = fmaf(a[4], bh.x, acc); acc = fmaf(a[5], bh.y, acc); acc = fmaf(a[6], bh.z, acc); acc = fmaf(a[7], bh.w, acc);
  return acc;
}
__device__ __forceinline__ float lt_sq8(const float* a, float acc) {
#pragma unroll
  for (int i = 0; i < 8; ++i) acc = fmaf(a[i], a[i], acc);
  return acc;
}

// lane i * T + t finishes (row i, column t): every lane holds every reduced sum
template <int T, int NR>
__device__ __forceinline__ void lt_finish(const float (&dot)[NR][T], const float (&xx)[NR], float* __restrict__ out,
                                          int row0, int lane, int D, double eps, double cap) {
  float d = 0.f, s = 0.f;
#pragma unroll
  for (int i = 0; i < NR; ++i)
#pragma unroll
    for (int t = 0; t < T; ++t)
      if (lane == i * T + t) { d = dot[i][t]; s = xx[i]; }
  if (lane < NR * T) {
    const double z = (double)d / sqrt((double)s / (double)D + eps);
    out[(size_t)row0 * T + lane] = (float)(cap > 0.0 ? cap * tanh(z / cap) : z);
  }
}

// one row against its table block in global memory
template <int T>
__device__ __forceinline__ void lt_row_global(const uint16_t* __restrict__ hr, const float* __restrict__ vb,
                                              float* __restrict__ out, int row, int lane, int D, double eps,
                                              double cap) {
  const int nvec = D >> 3;
  float dot[1][T], xx[1] = {0.f};
#pragma unroll
  for (int t = 0; t < T; ++t) dot[0][t] = 0.f;
  for (int c = lane; c < nvec; c += 64) {
    float f[8];
    unpack8(*reinterpret_cast<const uint4*>(hr + c * 8), f);
    xx[0] = lt_sq8(f, xx[0]);
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const float4* p = reinterpret_cast<const float4*>(vb + (size_t)t * D + c * 8);
      const float4 vl = p[0], vh = p[1];
      dot[0][t] = lt_dot8(f, vl, vh, dot[0][t]);
    }
  }
  xx[0] = wave_sum(xx[0]);
#pragma unroll
  for (int t = 0; t < T; ++t) dot[0][t] = wave_sum(dot[0][t]);
  lt_finish<T, 1>(dot, xx, out, row, lane, D, eps, cap);
}

// this thread's 16-byte pieces of the chunk at group g0 of table block vb (piece idx = tid + k * LT_THREADS: column
// t = idx / 128, group g = (idx % 128) / 2, half p = idx % 2), global -> registers
template <int T, int NS>
__device__ __forceinline__ void lt_fetch(float4 (&st)[NS], const float* __restrict__ vb, int g0, int nvec, int D,
                                         int tid) {
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int idx = tid + k * LT_THREADS;
    const int t = idx / (2 * LT_CHUNK), f = idx % (2 * LT_CHUNK), g = f >> 1, p = f & 1;
    st[k] = (idx < T * 2 * LT_CHUNK && g0 + g < nvec)
                ? *reinterpret_cast<const float4*>(vb + (size_t)t * D + (size_t)(g0 + g) * 8 + p * 4)
                : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// LDS image of a chunk: for column t, plane 0 holds the first and plane 1 the second 16 bytes of every 8-column
// group, 64 groups each, so both ds_read_b128 of a lane are lane-contiguous (no bank conflicts).
template <int T>
__global__ void __launch_bounds__(LT_THREADS) lens_track_kernel(
    const uint16_t* __restrict__ H, const float* __restrict__ V, const int32_t* __restrict__ vrow,
    float* __restrict__ out, int M, int U, int D, double eps, double cap) {
  __shared__ __attribute__((aligned(16))) float vs[T * 2 * LT_CHUNK * 4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nvec = D >> 3;
  const int wg0 = blockIdx.x * LT_ROWS;            // < M by the grid
  const int r0 = wg0 + wid * LT_RPW;
  int u0 = vrow[wg0];
  if (u0 < 0 || u0 >= U) u0 = -1;
  // the wave's four rows all exist and use the staged block (wave-uniform)
  bool fast = u0 >= 0 && r0 + LT_RPW <= M;
  if (fast) {
#pragma unroll
    for (int i = 0; i < LT_RPW; ++i) fast = fast && vrow[r0 + i] == u0;
  }

  if (u0 >= 0) {                                    // workgroup-uniform: the barriers below are reached by all
    const float* vb = V + (size_t)u0 * T * D;
    float dot[LT_RPW][T], xx[LT_RPW];
#pragma unroll
    for (int i = 0; i < LT_RPW; ++i) {
      xx[i] = 0.f;
#pragma unroll
      for (int t = 0; t < T; ++t) dot[i][t] = 0.f;
    }
    // the table piece of a chunk travels global -> registers -> LDS; the next chunk's piece and this chunk's rows are
    // in flight while the workgroup waits at the barriers and computes (one workgroup per CU at small M: nothing
    // else hides the latency)
    constexpr int NS = (T * 2 * LT_CHUNK + LT_THREADS - 1) / LT_THREADS;
    float4 st[NS];
    lt_fetch<T, NS>(st, vb, 0, nvec, D, tid);
    for (int g0 = 0; g0 < nvec; g0 += LT_CHUNK) {
      const int c = g0 + lane;
      const bool mine = fast && c < nvec;
      uint4 raw[LT_RPW];
      if (mine) {
#pragma unroll
        for (int i = 0; i < LT_RPW; ++i) raw[i] = *reinterpret_cast<const uint4*>(H + (size_t)(r0 + i) * D + c * 8);
      }
      if (g0) __syncthreads();                      // the previous chunk has been read
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        const int idx = tid + k * LT_THREADS;
        const int t = idx / (2 * LT_CHUNK), f = idx % (2 * LT_CHUNK), g = f >> 1, p = f & 1;
        if (idx < T * 2 * LT_CHUNK && g0 + g < nvec)
          *reinterpret_cast<float4*>(vs + ((t * 2 + p) * LT_CHUNK + g) * 4) = st[k];
      }
      __syncthreads();
      if (g0 + LT_CHUNK < nvec) lt_fetch<T, NS>(st, vb, g0 + LT_CHUNK, nvec, D, tid);
      if (mine) {
        float f[LT_RPW][8];
#pragma unroll
        for (int i = 0; i < LT_RPW; ++i) {
          unpack8(raw[i], f[i]);
          xx[i] = lt_sq8(f[i], xx[i]);
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
          const float4 vl = *reinterpret_cast<const float4*>(vs + ((t * 2 + 0) * LT_CHUNK + lane) * 4);
          const float4 vh = *reinterpret_cast<const float4*>(vs + ((t * 2 + 1) * LT_CHUNK + lane) * 4);
#pragma unroll
          for (int i = 0; i < LT_RPW; ++i) dot[i][t] = lt_dot8(f[i], vl, vh, dot[i][t]);
        }
      }
    }
    if (fast) {
#pragma unroll
      for (int i = 0; i < LT_RPW; ++i) {
        xx[i] = wave_sum(xx[i]);
#pragma unroll
        for (int t = 0; t < T; ++t) dot[i][t] = wave_sum(dot[i][t]);
      }
      lt_finish<T, LT_RPW>(dot, xx, out, r0, lane, D, eps, cap);
      return;
    }
  }
  // the wave's rows one at a time (no barrier past this point)
  for (int i = 0; i < LT_RPW; ++i) {
    const int r = r0 + i;
    if (r >= M) break;
    const int u = vrow[r];
    if (u < 0 || u >= U) {
      if (lane < T) out[(size_t)r * T + lane] = 0.f;
      continue;
    }
    lt_row_global<T>(H + (size_t)r * D, V + (size_t)u * T * D, out, r, lane, D, eps, cap);
  }
}

}  // namespace

int tb_lens_track(const uint16_t* h, const float* V, const int32_t* vrow, float* out, int M, int U, int T, int D,
                  double eps, double cap, hipStream_t st) {
  if (T < 1 || T > 8 || D < 8 || (D & 7) || D > 4096 || U < 0 || M < 0) return 3;
  if (M == 0) return 0;
  const dim3 grid((M + LT_ROWS - 1) / LT_ROWS), block(LT_THREADS);
#define TB_LT(TT) \
  case TT: hipLaunchKernelGGL((lens_track_kernel<TT>), grid, block, 0, st, h, V, vrow, out, M, U, D, eps, cap); break
  switch (T) {
    TB_LT(1); TB_LT(2); TB_LT(3); TB_LT(4); TB_LT(5); TB_LT(6); TB_LT(7); TB_LT(8);
  }
#undef TB_LT
  return 0;
}
