// Vocabulary-side readouts over bf16 logits [R, V] (SURVEY K10, K11, K12, K16,
// K17, K23).  The unembedding GEMM itself runs on hipBLASLt; everything that
// the reference does afterwards on the host over 1.6 GB fp32 arrays
// (`src/models.py:135-153`, `src/01_reproduce_logit_lens.py:35-71,147-149`)
// happens here on the device, so only [V]-sized results ever leave the GPU.
//
//  argmax_rows    greedy next token (optionally with the bf16 final-softcap
//                 rounding chain of HF generate, which can create ties)
//  row_lse        per-row log-sum-exp (online max/sum; logit-lens softmax)
//  gather_probs   p(row, id) = exp(z - lse) for secret / decoy ids
//  lens_colsum    acc[b, v] (+)= sum_t mask[b,t] * softmax(z[b,t])[v] with the
//                 reference's per-position id exclusions (2 ids per row)
//  topk_rows      per-row top-k (k <= 64), ties -> lower index
//  xent_rows      NLL of target ids under softcapped logits (fluency ΔNLL)
//  decode_head    one pass over a decode row: greedy token (argmax_rows semantics), its NLL and
//                 the NLL of an optional teacher target (the baseline's token at that column)
//  decode_head_track  decode_head plus the log-prob and rank of up to 8 tracked vocab ids per row (the sweep's
//                 output-side readout), counted in the same streamed pass
//  head_shift     KL(base || edit) and KL(edit || base) of an edited logits row against its baseline row (the
//                 sweep's output-shift readout), one streamed pass over both rows
//  head_movers    total variation between the two distributions of selected rows and the k tokens that gained /
//                 lost the most probability (the sweep's output-movers readout), two streamed passes
#include "common.h"
#include "api.h"
#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace {

// tanh for the final-logit softcap: 1 - 2/(e^{2|y|} + 1) on v_exp_f32 + v_rcp_f32 (a few fp32 ulp; the
// result is rounded to bf16 right after, like HF's bf16 tanh), odd Taylor series near 0 where that
// form cancels.  ~4x cheaper than libm tanhf, which made the 256k-wide vocab passes VALU-bound.
__device__ __forceinline__ float fast_tanh(float y) {
  const float a = fabsf(y);
  float t;
  if (a < 0.0625f) {
    const float a2 = a * a;
    t = a * (1.f + a2 * (-0.33333334f + a2 * 0.13333334f));
  } else {
    const float e = __expf(2.f * a);
    t = 1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f);
  }
  return copysignf(t, y);
}

__device__ __forceinline__ float softcap_bf16(float x, float cap) {
  // HF: logits / cap ; tanh ; * cap, each on a bf16 tensor.
  return rbf(rbf(fast_tanh(rbf(x / cap))) * cap);
}

// ---- exact bf16 softcap by table ------------------------------------------------------------
// softcap_bf16 is a pure function of its bf16 input bits and odd, so the 32768 results for the
// non-negative bit patterns (built on the host with the reference op, registered per cap value)
// make it one LDS lookup per element instead of ~25 VALU ops (the vocab-wide passes were
// VALU-bound on it).  Every kernel that applies the emulated softcap copies the 64 KB table to LDS.
constexpr int CTAB_N = 32768;

__device__ __forceinline__ const uint16_t* stage_ctab(const uint16_t* tab, uint16_t* lds) {
  if (tab == nullptr) return nullptr;
  for (int i = threadIdx.x; i < CTAB_N / 8; i += blockDim.x)
    reinterpret_cast<uint4*>(lds)[i] = reinterpret_cast<const uint4*>(tab)[i];
  __syncthreads();
  return lds;
}

__device__ __forceinline__ float ctab_get(const uint16_t* ct, uint32_t b) {
  return __uint_as_float(((uint32_t)ct[b & 0x7fffu] | (b & 0x8000u)) << 16);
}

// ---- compact exact softcap (decode_head) ------------------------------------------------------------------
// The chain rbf(rbf(tanh(rbf(x/cap))) * cap) equals rbf(rbf(x * (1/cap)) * cap) for |x| below `lo` (2.703 at cap 30:
// tanh(y) rounds to y there) and saturates at `sat` from `hi` on (104 at cap 30), both checked exhaustively against
// the reference table on the host (ops._softcap_table, tests/test_softcap_compact_cpu.py).  Only the hi - lo
// (~675) bit patterns in between need the table: 1.35 KB of LDS instead of 64 KB, read only by the lanes whose
// logit falls there — no bank-conflicted 64 KB gather, and the small LDS footprint lets full occupancy stream.
struct CapC {
  const uint16_t* tab;   // [hi - lo] bf16 magnitudes
  int lo, hi;
  float sat, rc, cap;
};
constexpr int CAPC_MAX = 2048;   // table entries staged (host-checked)

__device__ __forceinline__ float capc1(uint32_t b, const uint16_t* lt, const CapC& c) {
  const uint32_t ab = b & 0x7fffu;
  const float x = __uint_as_float(b << 16);
  const float a = rbf(rbf(x * c.rc) * c.cap);
  if (ab < (uint32_t)c.lo) return a;
  float mag;
  if (ab < (uint32_t)c.hi) mag = __uint_as_float((uint32_t)lt[ab - c.lo] << 16);
  else if (ab <= 0x7f80u) mag = c.sat;
  else return x;   // NaN stays NaN
  return (b & 0x8000u) ? -mag : mag;
}

// 8 logits of a uint4 -> capped fp32 (table, emulated compute, fp32 tanh, or none)
__device__ __forceinline__ void capped8(const uint4& v, float* f, const uint16_t* ct, float cap, int emu) {
  if (ct != nullptr) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      f[2 * k] = ctab_get(ct, w[k] & 0xffffu);
      f[2 * k + 1] = ctab_get(ct, w[k] >> 16);
    }
    return;
  }
  unpack8(v, f);
  if (cap > 0.f) {
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = emu ? softcap_bf16(f[j], cap) : fast_tanh(f[j] / cap) * cap;
  }
}

__device__ __forceinline__ float capped1(uint16_t b, const uint16_t* ct, float cap, int emu) {
  if (ct != nullptr) return ctab_get(ct, b);
  const float x = bf2f(b);
  if (cap <= 0.f) return x;
  return emu ? softcap_bf16(x, cap) : fast_tanh(x / cap) * cap;
}

// Streams one row's 16-B vectors c = tid, tid + stride, ... with UNR loads in flight per thread before the first
// is consumed: with the 64 KB softcap table in LDS only 2 blocks (16 waves) fit on a CU, and one outstanding 16-B
// load per lane cannot cover HBM latency.  f(v, c) runs in the plain loop's order (bit-identical reductions).
// (UNR = 1: the plain loop)
template <int UNR, typename F>
__device__ __forceinline__ void stream_row(const uint4* __restrict__ p, int nv, F&& f) {
  const int st = blockDim.x;
  int c = threadIdx.x;
  for (; c + (UNR - 1) * st < nv; c += UNR * st) {
    uint4 v[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) v[u] = p[c + u * st];
#pragma unroll
    for (int u = 0; u < UNR; ++u) f(v[u], c + u * st);
  }
  for (; c < nv; c += st) f(p[c], c);
}
constexpr int ROW_UNR = 4;   // (8 loads in flight per lane measured 2-5 % slower than 4: profiles/r3/dh5)

// ---- capping policies of the running-max row pass ---------------------------------------------------------
// stage() puts its table into LDS (block-wide, ends in a barrier where it copied), then
// cap8 / cap1 give the capped fp32 logits of a 16-B vector / of one bf16.
// CapRun: capped8 / capped1 with their runtime dispatch (64 KB table, emulated compute, fp32 tanh, or none).
struct CapRun {
  const uint16_t* ct;   // the registered table (or nullptr); after stage() its LDS copy
  float cap;
  int emu;
  __device__ __forceinline__ void stage() {
    extern __shared__ __attribute__((aligned(16))) uint16_t ctab_lds[];
    ct = stage_ctab(ct, ctab_lds);
  }
  __device__ __forceinline__ void cap8(const uint4& v, float* f) const { capped8(v, f, ct, cap, emu); }
  __device__ __forceinline__ float cap1(uint16_t b) const { return capped1(b, ct, cap, emu); }
};
// CapRunEmu: CapRun with emulate_bf16 a constant, as decode_head needs it (no fp32-tanh code in its kernel)
struct CapRunEmu : CapRun {
  __device__ __forceinline__ void cap8(const uint4& v, float* f) const { capped8(v, f, ct, cap, 1); }
  __device__ __forceinline__ float cap1(uint16_t b) const { return capped1(b, ct, cap, 1); }
};
// CapCompact: the compact softcap (see CapC) on its ~1.35 KB static LDS table
struct CapCompact {
  CapC c;
  const uint16_t* lt;   // set by stage()
  __device__ __forceinline__ void stage() {
    __shared__ __attribute__((aligned(16))) uint16_t lds[CAPC_MAX];
    for (int i = threadIdx.x; i < c.hi - c.lo; i += blockDim.x) lds[i] = c.tab[i];
    __syncthreads();
    lt = lds;
  }
  __device__ __forceinline__ void cap8(const uint4& v, float* f) const {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      f[2 * k] = capc1(w[k] & 0xffffu, lt, c);
      f[2 * k + 1] = capc1(w[k] >> 16, lt, c);
    }
  }
  __device__ __forceinline__ float cap1(uint16_t b) const { return capc1(b, lt, c); }
};

// ---- accumulators and their block reduction -----------------------------------------------------------------
// What a lane carries over its share of a row -- ArgBest, OnlineLse, plain float sums, integer counts -- each with
// merge(a, b) and shfl_xor(x, o), which is all that wave_reduce / block_reduce ask of a type.
struct ArgBest {
  float v;
  int i;
};
__device__ __forceinline__ ArgBest better(ArgBest a, ArgBest b) {
  if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}

// online log-sum-exp: max m (-inf: nothing seen yet) and s = sum exp(x - m)
struct OnlineLse {
  float m, s;
};
__device__ __forceinline__ void online_add(float& m, float& s, float x) {
  if (x > m) {
    s = s * __expf(m - x) + 1.f;
    m = x;
  } else {
    s += __expf(x - m);
  }
}
__device__ __forceinline__ void online_merge(float& m, float& s, float m2, float s2) {
  if (m2 == -INFINITY) return;
  if (m == -INFINITY) { m = m2; s = s2; return; }
  if (m2 > m) { s = s * __expf(m - m2) + s2; m = m2; }
  else { s += s2 * __expf(m2 - m); }
}

__device__ __forceinline__ ArgBest merge(ArgBest a, ArgBest b) { return better(a, b); }
__device__ __forceinline__ OnlineLse merge(OnlineLse a, OnlineLse b) {
  online_merge(a.m, a.s, b.m, b.s);
  return a;
}
__device__ __forceinline__ float merge(float a, float b) { return a + b; }
__device__ __forceinline__ int merge(int a, int b) { return a + b; }

__device__ __forceinline__ float shfl_xor(float x, int o) { return __shfl_xor(x, o, 64); }
__device__ __forceinline__ int shfl_xor(int x, int o) { return __shfl_xor(x, o, 64); }
__device__ __forceinline__ ArgBest shfl_xor(ArgBest x, int o) { return {shfl_xor(x.v, o), shfl_xor(x.i, o)}; }
__device__ __forceinline__ OnlineLse shfl_xor(OnlineLse x, int o) { return {shfl_xor(x.m, o), shfl_xor(x.s, o)}; }

// An accumulator's per-wave LDS slots (8 waves at most), one array per scalar: a struct's fields are stored apart,
// so no store or load needs a register pair (array-of-structs slots cost the track kernel an occupancy step)
template <typename T>
struct Slots {
  T x[8];
  __device__ __forceinline__ void put(int w, T a) { x[w] = a; }
  __device__ __forceinline__ T get(int w) const { return x[w]; }
};
template <>
struct Slots<ArgBest> {
  float v[8];
  int i[8];
  __device__ __forceinline__ void put(int w, ArgBest a) { v[w] = a.v; i[w] = a.i; }
  __device__ __forceinline__ ArgBest get(int w) const { return {v[w], i[w]}; }
};
template <>
struct Slots<OnlineLse> {
  float m[8], s[8];
  __device__ __forceinline__ void put(int w, OnlineLse a) { m[w] = a.m; s[w] = a.s; }
  __device__ __forceinline__ OnlineLse get(int w) const { return {m[w], s[w]}; }
};


// the wave's butterfly, xor 32 .. 1, over all accumulators side by side: every lane ends with the wave's value
template <typename... T>
__device__ __forceinline__ void wave_reduce(T&... x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ((x = merge(x, shfl_xor(x, o))), ...);
}

// An accumulator and its __shared__ slots, one per wave (8 at most), for block_reduce: the butterfly, lane 0 of each
// wave to the wave's slot, a barrier, then thread 0 folds the waves in order 0, 1, ... -- only thread 0 holds the
// block's values afterwards.  The order is part of every float result's bits.  A block that reduces again (the next
// row of a persistent kernel) needs a barrier of its own before it rewrites the slots.
template <typename T>
struct Red {
  T& x;
  Slots<T>& slot;
};
template <typename T>
__device__ __forceinline__ Red<T> red(T& x, Slots<T>& slot) { return {x, slot}; }

template <typename... T>
__device__ __forceinline__ void block_reduce(Red<T>... r) {
  wave_reduce(r.x...);
  if ((threadIdx.x & 63) == 0) (r.slot.put(threadIdx.x >> 6, r.x), ...);
  __syncthreads();
  if (threadIdx.x == 0) {
    ((r.x = r.slot.get(0)), ...);
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) ((r.x = merge(r.x, r.slot.get(w))), ...);
  }
}

__global__ void __launch_bounds__(512) argmax_rows_kernel(const uint16_t* __restrict__ logits,
                                                          int32_t* __restrict__ out, int V, float cap,
                                                          const uint16_t* __restrict__ tab) {
  __shared__ Slots<ArgBest> sb;
  extern __shared__ __attribute__((aligned(16))) uint16_t ctab_lds[];
  const uint16_t* ct = stage_ctab(tab, ctab_lds);
  const uint16_t* row = logits + (size_t)blockIdx.x * V;
  ArgBest best{-INFINITY, 0x7fffffff};
  const int nv = V >> 3;
  stream_row<ROW_UNR>(reinterpret_cast<const uint4*>(row), nv, [&](const uint4& v, int c) {
    float f[8];
    capped8(v, f, ct, cap, 1);
#pragma unroll
    for (int j = 0; j < 8; ++j) best = better(best, ArgBest{f[j], c * 8 + j});
  });
  for (int c = nv * 8 + threadIdx.x; c < V; c += blockDim.x) {
    const float x = capped1(row[c], ct, cap, 1);
    best = better(best, ArgBest{x, c});
  }
  block_reduce(red(best, sb));
  if (threadIdx.x == 0) out[blockIdx.x] = best.i;
}

// One lane's share of a row's online log-sum-exp under capping policy ``cp``: the streamed 8-wide step (local max,
// local exp-sum, one online_merge per vector), then the V % 8 tail column by column.  each(x, col) also sees
// every capped logit, in the same order.
template <typename Cap, typename Each>
__device__ __forceinline__ OnlineLse lse_row(const uint16_t* row, int V, const Cap& cp, Each&& each) {
  OnlineLse l{-INFINITY, 0.f};
  const int nv = V >> 3;
  stream_row<ROW_UNR>(reinterpret_cast<const uint4*>(row), nv, [&](const uint4& v, int c) {
    float f[8];
    cp.cap8(v, f);
    float lm = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      lm = fmaxf(lm, f[j]);
      each(f[j], c * 8 + j);
    }
    float ls = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) ls += __expf(f[j] - lm);
    online_merge(l.m, l.s, lm, ls);
  });
  for (int c = nv * 8 + threadIdx.x; c < V; c += blockDim.x) {
    const float x = cp.cap1(row[c]);
    each(x, c);
    if (l.m == -INFINITY) { l.m = x; l.s = 1.f; } else online_add(l.m, l.s, x);
  }
  return l;
}
__device__ __forceinline__ float lse_of(OnlineLse l) { return l.m + __logf(l.s); }

__global__ void __launch_bounds__(512) row_lse_kernel(const uint16_t* __restrict__ logits, float* __restrict__ lse,
                                                      int V, float cap, int emulate_bf16,
                                                      const uint16_t* __restrict__ tab) {
  __shared__ Slots<OnlineLse> sl;
  CapRun cp{tab, cap, emulate_bf16};
  cp.stage();
  OnlineLse l = lse_row(logits + (size_t)blockIdx.x * V, V, cp, [](float, int) {});
  block_reduce(red(l, sl));
  if (threadIdx.x == 0) lse[blockIdx.x] = lse_of(l);
}

// ``rowmap`` (optional): logical row r reads logits / lse row rowmap[r] (rows deduplicated upstream).
__global__ void gather_probs_kernel(const uint16_t* __restrict__ logits, const float* __restrict__ lse,
                                    const int32_t* __restrict__ ids, float* __restrict__ out, int R, int K, int V,
                                    int round_bf16, const int32_t* __restrict__ rowmap) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= R * K) return;
  const int r = rowmap ? rowmap[e / K] : e / K;
  const int id = ids[e];
  if (id < 0 || id >= V) { out[e] = 0.f; return; }
  float p = __expf(bf2f(logits[(size_t)r * V + id]) - lse[r]);
  out[e] = round_bf16 ? rbf(p) : p;
}

// grid (ceil(V / (8*256)), B); rows of sequence b are b*T .. b*T+T-1.
// Rows of sequence b: [b*T, b*T+T) (dense, mask may skip rows) or [offs[b], offs[b+1]) (packed).
// With ``cum`` the running sum after each row is also written to cum[b, t+1, :] (cum[b, 0] = start),
// so later consumers can take any prefix sum of a sequence's lens probabilities with one row read.
__global__ void __launch_bounds__(256) lens_colsum_kernel(const uint16_t* __restrict__ logits,
                                                          const float* __restrict__ lse,
                                                          const uint8_t* __restrict__ mask,
                                                          const int32_t* __restrict__ excl, float* __restrict__ acc,
                                                          int T, int V, int accumulate, int round_bf16,
                                                          const int32_t* __restrict__ offs, float* __restrict__ cum,
                                                          const int32_t* __restrict__ rowmap) {
  const int b = blockIdx.y;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;   // 8-column group
  const int col0 = c * 8;
  if (col0 >= V) return;
  const bool full = col0 + 8 <= V;
  float a[8];
  float* dst = acc + (size_t)b * V + col0;
  if (accumulate && full) {
    const float4 x0 = reinterpret_cast<const float4*>(dst)[0], x1 = reinterpret_cast<const float4*>(dst)[1];
    a[0] = x0.x; a[1] = x0.y; a[2] = x0.z; a[3] = x0.w; a[4] = x1.x; a[5] = x1.y; a[6] = x1.z; a[7] = x1.w;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = (accumulate && col0 + j < V) ? dst[j] : 0.f;
  }
  auto put = [&](float* d) {
    if (full) {
      reinterpret_cast<float4*>(d)[0] = make_float4(a[0], a[1], a[2], a[3]);
      reinterpret_cast<float4*>(d)[1] = make_float4(a[4], a[5], a[6], a[7]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (col0 + j < V) d[j] = a[j];
    }
  };
  const int r0 = offs ? offs[b] : b * T, r1 = offs ? offs[b + 1] : b * T + T;
  float* cb = cum ? cum + (size_t)b * (T + 1) * V + col0 : nullptr;
  if (cb) put(cb);
  for (int r = r0; r < r1; ++r) {
    if (mask == nullptr || mask[r]) {
      const int pr = rowmap ? rowmap[r] : r;             // physical logits row (deduplicated rows)
      const float l = lse[pr];
      const int e0 = excl[2 * r], e1 = excl[2 * r + 1];
      const uint16_t* row = logits + (size_t)pr * V;
      float f[8];
      if (full) {
        unpack8(*reinterpret_cast<const uint4*>(row + col0), f);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = (col0 + j < V) ? bf2f(row[col0 + j]) : -INFINITY;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float p = __expf(f[j] - l);
        if (round_bf16) p = rbf(p);
        const int id = col0 + j;
        if (id == e0 || id == e1) p = 0.f;
        a[j] += p;
      }
    }
    if (cb) put(cb + (size_t)(r - r0 + 1) * V);
  }
  put(dst);
}

// Per-row top-k by k rounds of block argmax over per-thread sorted candidate lists (ties: lower column first).
// Workgroup b takes chunk b % C (CH columns) of row b / C and writes its k best to vals / idx[b * K ..]; with xi the
// row holds candidates whose columns are xi (the second pass of a chunked top-k: the same order, so the same set).
template <int KMAX>
__global__ void __launch_bounds__(256) topk_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ xi,
                                                        float* __restrict__ vals, int32_t* __restrict__ idx, int V,
                                                        int K, int CH, int C) {
  __shared__ float sv[4];
  __shared__ int si[4];
  __shared__ int win;
  const int r = blockIdx.x / C, ch = blockIdx.x - r * C;
  const float* row = x + (size_t)r * V;
  const int32_t* rowi = xi != nullptr ? xi + (size_t)r * V : nullptr;
  const int cend = min(V, (ch + 1) * CH);
  float tv[KMAX];
  int ti[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) { tv[j] = -INFINITY; ti[j] = 0x7fffffff; }
  // the list's last entry in registers: the common case (no insertion) reads no dynamically indexed list entry
  float thv = -INFINITY;
  int thi = 0x7fffffff;
  auto ins = [&](float v, int c) {
    if (!(v > thv || (v == thv && c < thi))) return;
    // insertion into the sorted list (descending, ties by lower index first) as an unrolled shift network: every
    // list index is a compile-time constant (a loop with a per-lane index became a waterfall over the lanes)
#pragma unroll
    for (int j = KMAX - 1; j >= 0; --j) {
      const bool here = v > tv[j] || (v == tv[j] && c < ti[j]);
      bool above = false;
      if (j > 0) above = v > tv[j - 1] || (v == tv[j - 1] && c < ti[j - 1]);
      if (j > 0 && above) { tv[j] = tv[j - 1]; ti[j] = ti[j - 1]; }
      else if (here) { tv[j] = v; ti[j] = c; }
    }
    thv = tv[K - 1];
    thi = ti[K - 1];
  };
  const int cbeg = ch * CH;
  if (rowi == nullptr && (V & 3) == 0 && (CH & 3) == 0) {
    // 16-B loads, 4 in flight per thread before any compare
    const float4* row4 = reinterpret_cast<const float4*>(row);
    const int b4 = cbeg >> 2, e4 = cend >> 2;
    for (int p = b4 + threadIdx.x; p < e4; p += 4 * blockDim.x) {
      float4 a[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = p + u * blockDim.x;
        a[u] = q < e4 ? row4[q] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = 4 * (p + u * blockDim.x);
        if (c >= cend) break;
        ins(a[u].x, c);
        ins(a[u].y, c + 1);
        ins(a[u].z, c + 2);
        ins(a[u].w, c + 3);
      }
    }
  } else {
    for (int p = cbeg + threadIdx.x; p < cend; p += blockDim.x) ins(row[p], rowi != nullptr ? rowi[p] : p);
  }
  // K rounds of block argmax over the lists' heads; the winning list shifts left (constant indices, as above).
  // Entries past K are dropped first, so a list never offers more than its K best.
#pragma unroll
  for (int j = 0; j < KMAX; ++j)
    if (j >= K) { tv[j] = -INFINITY; ti[j] = 0x7fffffff; }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int k = 0; k < K; ++k) {
    ArgBest b{tv[0], ti[0]};
    // ties: prefer lower index
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      ArgBest oth{__shfl_xor(b.v, o, 64), __shfl_xor(b.i, o, 64)};
      b = better(b, oth);
    }
    if (lane == 0) { sv[wid] = b.v; si[wid] = b.i; }
    __syncthreads();
    if (threadIdx.x == 0) {
      ArgBest bb{sv[0], si[0]};
      for (int w = 1; w < 4; ++w) bb = better(bb, ArgBest{sv[w], si[w]});
      vals[(size_t)blockIdx.x * K + k] = bb.v;
      idx[(size_t)blockIdx.x * K + k] = bb.i;
      win = bb.i;
    }
    __syncthreads();
    if (ti[0] == win) {
#pragma unroll
      for (int j = 0; j + 1 < KMAX; ++j) { tv[j] = tv[j + 1]; ti[j] = ti[j + 1]; }
      tv[KMAX - 1] = -INFINITY;
      ti[KMAX - 1] = 0x7fffffff;
    }
    __syncthreads();
  }
}

// row_lse minus the capped target logit; a target outside [0, V) writes 0 and stages nothing
__global__ void __launch_bounds__(512) xent_rows_kernel(const uint16_t* __restrict__ logits,
                                                        const int32_t* __restrict__ tgt, float* __restrict__ nll,
                                                        int V, float cap, int emulate_bf16,
                                                        const uint16_t* __restrict__ tab) {
  __shared__ Slots<OnlineLse> sl;
  const int r = blockIdx.x;
  const int t = tgt[r];
  if (t < 0 || t >= V) {
    if (threadIdx.x == 0) nll[r] = 0.f;
    return;
  }
  CapRun cp{tab, cap, emulate_bf16};
  cp.stage();
  const uint16_t* row = logits + (size_t)r * V;
  OnlineLse l = lse_row(row, V, cp, [](float, int) {});
  block_reduce(red(l, sl));
  if (threadIdx.x == 0) nll[r] = lse_of(l) - cp.cap1(row[t]);
}

// What thread 0 writes for row r of a decode_head pass: the greedy token, its NLL and, with nll_tgt, the NLL of the
// teacher target (0 for a target outside [0, V)).  zt(t): the capped logit of column t.
template <typename Zt>
__device__ __forceinline__ void head_write(int r, float lse, ArgBest b, const int32_t* __restrict__ tgt,
                                           int32_t* __restrict__ nxt, float* __restrict__ nll_self,
                                           float* __restrict__ nll_tgt, int V, Zt&& zt) {
  nxt[r] = b.i;
  nll_self[r] = lse - b.v;
  if (nll_tgt != nullptr) {
    const int t = tgt[r];
    nll_tgt[r] = (t >= 0 && t < V) ? lse - zt(t) : 0.f;
  }
}

// decode_head with a running max, one block per row: every cap the fixed-offset kernel below does not take, and
// TB_DECODE_HEAD=t / c.  CapRunEmu and CapCompact give the same capped values in the same order, so the same outputs.
template <typename Cap>
__global__ void __launch_bounds__(512) decode_head_kernel(const uint16_t* __restrict__ logits,
                                                          const int32_t* __restrict__ tgt, int32_t* __restrict__ nxt,
                                                          float* __restrict__ nll_self, float* __restrict__ nll_tgt,
                                                          int V, Cap cp) {
  __shared__ Slots<OnlineLse> sl;
  __shared__ Slots<ArgBest> sb;
  cp.stage();
  const int r = blockIdx.x;
  const uint16_t* row = logits + (size_t)r * V;
  ArgBest best{-INFINITY, 0x7fffffff};
  OnlineLse l = lse_row(row, V, cp, [&](float x, int c) { best = better(best, ArgBest{x, c}); });
  block_reduce(red(l, sl), red(best, sb));
  if (threadIdx.x == 0)
    head_write(r, lse_of(l), best, tgt, nxt, nll_self, nll_tgt, V, [&](int t) { return cp.cap1(row[t]); });
}

// decode_head for 0 < cap <= DH_FIXED_CAP, the default: the same outputs as decode_head_kernel (argmax bit-exact,
// NLLs to fp32 summation order) on about half the VALU work per logit, which is what bound the row pass
// (2.9 TB/s).  (1) Capped logits lie in [-cap, cap], so sum(exp(z)) over the row can neither
// overflow nor underflow in fp32: no running max, no rescaling, one exp + add per logit.  (2) The argmax keeps
// the best 8-logit chunk (its max against the thread's best, strict > so the earliest chunk wins) and resolves
// the index inside the winning chunk once per row by re-reading its 16 B — first index of the max, as torch.
// (3) Persistent: 2 blocks per CU loop over the rows, so the 64 KB table is staged once per block instead of once
// per row (+12.5 % HBM/L2 traffic at the Gemma-2 vocab).
constexpr float DH_FIXED_CAP = 40.f;   // e^40 * 2^20 columns < FLT_MAX; e^-40 a normal float

// 8 capped logits of a uint4 through the 64 KB table at ~4 VALU ops per logit (the generic capped8 path costs ~5):
// the 15-bit magnitudes come from v_bfe (opaque to the compiler, which otherwise rewrites the index math into three
// ops), the two lookups of a dword are packed with one v_lshl_or, one v_and_or puts both signs back, a shift / a
// mask unpack them.  (ds_read_u16_d16_hi cannot pack them: with SRAM ECC on, d16 loads zero the other half.)
__device__ __forceinline__ void capped8_tab(const uint4& v, float* f, const uint16_t* ct) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t ilo, ihi, q;
    asm("v_bfe_u32 %0, %1, 0, 15" : "=v"(ilo) : "v"(w[k]));
    asm("v_bfe_u32 %0, %1, 16, 15" : "=v"(ihi) : "v"(w[k]));
    const uint32_t p = ((uint32_t)ct[ihi] << 16) | ct[ilo];   // table entries are magnitudes (bit 15 clear)
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(q) : "v"(w[k]), "s"(0x80008000u), "v"(p));
    f[2 * k] = __uint_as_float(q << 16);
    f[2 * k + 1] = __uint_as_float(q & 0xffff0000u);
  }
}

// v_max3_f32 / v_max_f32 without the canonicalising v_max x, x the compiler puts before fmaxf on bit-cast inputs
// (table values are never signalling NaNs)
__device__ __forceinline__ float max3_raw(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ float fmax_raw(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
typedef float f2 __attribute__((ext_vector_type(2)));
constexpr f2 LOG2E2 = {1.4426950408889634f, 1.4426950408889634f};

// One lane's share of a row on the fixed-offset path (decode_head_f_kernel and decode_head_track_kernel run these
// statements, so their nxt / nll_self / nll_tgt have the same bits): the exp-sum as two packed halves and the best
// 8-logit chunk; finish() turns them into the lane's sum and ArgBest.
struct FixedAcc {
  f2 s2 = {0.f, 0.f};
  float bv = -INFINITY;
  int bc = -1;

  // the 8 logits of vector c; their capped values stay in f for the caller
  __device__ __forceinline__ void chunk(const uint4& v, int c, const uint16_t* ct, float* f) {
    capped8_tab(v, f, ct);
    const float cm = max3_raw(max3_raw(f[0], f[1], f[2]), max3_raw(f[3], f[4], f[5]), fmax_raw(f[6], f[7]));
#pragma unroll
    for (int j = 0; j < 8; j += 2) {   // packed scale / add (v_pk_mul_f32, v_pk_add_f32), exp2 per lane
      const f2 y = f2{f[j], f[j + 1]} * LOG2E2;
      s2 += f2{__builtin_amdgcn_exp2f(y.x), __builtin_amdgcn_exp2f(y.y)};
    }
    if (cm > bv) { bv = cm; bc = c; }
  }

  // after the stream: the index inside the winning chunk (re-read; the first of the maxima), then the V % 8 tail
  // column by column; tail(x) also sees each tail column's capped logit
  template <typename Tail>
  __device__ __forceinline__ void finish(const uint16_t* row, int V, const uint16_t* ct, float& s, ArgBest& best,
                                         Tail&& tail) const {
    s = s2.x + s2.y;
    best = ArgBest{bv, 0x7fffffff};
    if (bc >= 0) {
      float f[8];
      capped8(reinterpret_cast<const uint4*>(row)[bc], f, ct, 0.f, 1);
#pragma unroll
      for (int j = 7; j >= 0; --j)
        if (f[j] == bv) best.i = bc * 8 + j;
    }
    for (int c = (V >> 3) * 8 + threadIdx.x; c < V; c += blockDim.x) {
      const float x = capped1(row[c], ct, 0.f, 1);
      s += __expf(x);
      best = better(best, ArgBest{x, c});
      tail(x);
    }
  }
};

// stats != nullptr (vocab-parallel TP head, models/gemma2.py): instead of the token / NLLs, per row the float4
// {log-sum-exp, best capped logit, its global vocab id (local + off), the capped logit of the teacher target
// tgt - off if it falls in this rank's [0, V) slice, else -inf}, merged over the ranks by vp_head_merge (vp.hip)
template <int UNR>
__global__ void __launch_bounds__(512) decode_head_f_kernel(const uint16_t* __restrict__ logits,
                                                            const int32_t* __restrict__ tgt, int32_t* __restrict__ nxt,
                                                            float* __restrict__ nll_self, float* __restrict__ nll_tgt,
                                                            int R, int V, const uint16_t* __restrict__ tab,
                                                            float4* __restrict__ stats, int off) {
  __shared__ Slots<float> ss;
  __shared__ Slots<ArgBest> sb;
  extern __shared__ __attribute__((aligned(16))) uint16_t ctab_lds[];
  const uint16_t* ct = stage_ctab(tab, ctab_lds);
  for (int r = blockIdx.x; r < R; r += gridDim.x) {
    const uint16_t* row = logits + (size_t)r * V;
    FixedAcc a;
    stream_row<UNR>(reinterpret_cast<const uint4*>(row), V >> 3, [&](const uint4& v, int c) {
      float f[8];
      a.chunk(v, c, ct, f);
    });
    float s;
    ArgBest best;
    a.finish(row, V, ct, s, best, [](float) {});
    block_reduce(red(s, ss), red(best, sb));
    if (threadIdx.x == 0) {
      const float lse = __logf(s);
      if (stats != nullptr) {
        const int t = tgt != nullptr ? tgt[r] - off : -1;
        const float tl = (tgt != nullptr && tgt[r] >= 0 && t >= 0 && t < V) ? capped1(row[t], ct, 0.f, 1) : -INFINITY;
        stats[r] = make_float4(lse, best.v, (float)(best.i + off), tl);   // vocab ids < 2^24: exact in fp32
      } else {
        head_write(r, lse, best, tgt, nxt, nll_self, nll_tgt, V, [&](int t) { return capped1(row[t], ct, 0.f, 1); });
      }
    }
    __syncthreads();   // the slots are rewritten by the next row
  }
}

// decode_head_f_kernel (plain mode) plus the output-side readout of T <= DH_TRACK_MAX tracked vocab ids per row:
// logp = capped logit - lse, and for the first n_rank <= NR columns the rank #{v : c(z[v]) > c(z[id])} (strict, so a
// saturated tie group shares rank 0).  The ranked columns' logits are read before the stream (broadcast loads).  The
// exp-sum and the chunk argmax are the plain kernel's (FixedAcc, head_write), so nxt / nll_self / nll_tgt keep its
// bits; the compares ride along on the same capped floats.  Counting costs one VALU op per logit and ranked column:
// v_cmp_gt_f32 against the wave-uniform threshold writes the wave's lane mask to an SGPR pair, and the population
// count and the add run on the scalar unit beside the vector stream (no packed f32 compare exists, and packed 16-bit
// keys would cost 1.5 ops per logit for the key before the first column).  The ballot counts a whole wave, so it is
// used only in trips that every lane of the wave runs (the trip count is the wave's, not the lane's); the ragged
// rest of a row -- at most UNR chunks per lane and the V % 8 tail -- is counted per lane and folded by the wave
// reduction.  The count is an integer, so any merge order gives the same value.
// Columns k >= n_rank inside NR compare against +inf.  With ``col`` row r writes column min(col[r], W - 1) of
// [R, W, T] outputs (the decode's per-step columns) instead of [R, T].
constexpr int DH_TRACK_MAX = 8;
struct HeadTrack {
  const int32_t* ids;   // [R, T], -1 (any id outside [0, V)) = empty column
  float* logp;
  int32_t* rank;
  const int64_t* col;   // optional [R]
  int T, n_rank, W;
};

template <int NR>
__global__ void __launch_bounds__(512) decode_head_track_kernel(const uint16_t* __restrict__ logits,
                                                                const int32_t* __restrict__ tgt,
                                                                int32_t* __restrict__ nxt, float* __restrict__ nll_self,
                                                                float* __restrict__ nll_tgt, int R, int V,
                                                                const uint16_t* __restrict__ tab, HeadTrack tk) {
  __shared__ Slots<float> ss;
  __shared__ Slots<ArgBest> sb;
  __shared__ int sc[8][NR > 0 ? NR : 1];
  extern __shared__ __attribute__((aligned(16))) uint16_t ctab_lds[];
  const uint16_t* ct = stage_ctab(tab, ctab_lds);
  const int nv = V >> 3;
  for (int r = blockIdx.x; r < R; r += gridDim.x) {
    const uint16_t* row = logits + (size_t)r * V;
    // thresholds of the ranked columns (+inf: empty or unranked, nothing counts); only these stay live over the stream
    float thr[NR > 0 ? NR : 1];
    int wcnt[NR > 0 ? NR : 1];   // counted by the whole wave (full trips), wave-uniform
    int lcnt[NR > 0 ? NR : 1];   // counted by this lane alone (ragged trips)
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      const int id = k < tk.n_rank ? tk.ids[(size_t)r * tk.T + k] : -1;
      thr[k] = (id >= 0 && id < V) ? capped1(row[id], ct, 0.f, 1) : INFINITY;
      wcnt[k] = 0;
      lcnt[k] = 0;
    }
    FixedAcc a;
    // stream_row's order per lane (c = tid, tid + stride, ...: the same reductions), split by the wave instead of by
    // the lane: UNR-deep trips run while the wave's LAST lane still has all UNR chunks, so every lane is active in
    // them and the ballot counts the whole wave; what is left (up to UNR chunks per lane, ragged over the lanes) is
    // counted per lane
    {
      constexpr int UNR = ROW_UNR;
      const uint4* p = reinterpret_cast<const uint4*>(row);
      const int st = blockDim.x;
      int c = threadIdx.x;
      int cw = __builtin_amdgcn_readfirstlane(threadIdx.x) + 63;
      for (; cw + (UNR - 1) * st < nv; cw += UNR * st, c += UNR * st) {
        uint4 v[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) v[u] = p[c + u * st];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          float f[8];
          a.chunk(v[u], c + u * st, ct, f);
#pragma unroll
          for (int k = 0; k < NR; ++k) {
#pragma unroll
            for (int j = 0; j < 8; ++j) wcnt[k] += __builtin_popcountll(__builtin_amdgcn_ballot_w64(f[j] > thr[k]));
          }
          if (NR > 0) __builtin_amdgcn_sched_barrier(0);   // the lane masks of one chunk, not of UNR, live in SGPRs
        }
      }
      for (; c < nv; c += st) {
        float f[8];
        a.chunk(p[c], c, ct, f);
#pragma unroll
        for (int k = 0; k < NR; ++k) {
#pragma unroll
          for (int j = 0; j < 8; ++j) lcnt[k] += f[j] > thr[k] ? 1 : 0;
        }
      }
    }
    float s;
    ArgBest best;
    a.finish(row, V, ct, s, best, [&](float x) {
#pragma unroll
      for (int k = 0; k < NR; ++k) lcnt[k] += x > thr[k] ? 1 : 0;
    });
    // a wave's count goes to its own slot: the waves are added up only for the columns that get a rank (below)
#pragma unroll
    for (int k = 0; k < NR; ++k) wave_reduce(lcnt[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < NR; ++k) sc[threadIdx.x >> 6][k] = wcnt[k] + lcnt[k];
    }
    block_reduce(red(s, ss), red(best, sb));   // its barrier publishes sc as well
    if (threadIdx.x == 0) {
      const float lse = __logf(s);
      head_write(r, lse, best, tgt, nxt, nll_self, nll_tgt, V, [&](int t) { return capped1(row[t], ct, 0.f, 1); });
      size_t o = (size_t)r;
      if (tk.col != nullptr) o = o * tk.W + (size_t)min(max(tk.col[r], (int64_t)0), (int64_t)(tk.W - 1));
      o *= tk.T;
      for (int k = 0; k < tk.T; ++k) {
        const int id = tk.ids[(size_t)r * tk.T + k];
        const bool ok = id >= 0 && id < V;
        int rk = -1;
        if (k < NR && k < tk.n_rank && ok) {
          rk = 0;
          for (int w = 0; w < (int)(blockDim.x >> 6); ++w) rk += sc[w][k];
        }
        tk.logp[o + k] = ok ? capped1(row[id], ct, 0.f, 1) - lse : 0.f;
        tk.rank[o + k] = rk;
      }
    }
    __syncthreads();   // the slots and sc are rewritten by the next row
  }
}

// Output shift of an edit: for row r with b = rowmap[r], q = c(logits[r]) and p = c(base[b]) (the capped logits
// decode_head_f_kernel sees, through the same LDS table), both KL divergences between the two next-token
// distributions from ONE streamed pass over the two rows:
//   S_p = sum e^p, S_q = sum e^q, A = sum e^p (p - q), B = sum e^q (q - p)
//   kl[r]     = KL(base || edit) = A / S_p - (ln S_p - ln S_q)
//   kl_rev[r] = KL(edit || base) = B / S_q + (ln S_p - ln S_q)
// Capped logits lie in [-cap, cap] with cap <= DH_FIXED_CAP, so the four sums need no running max (|A|, |B| <=
// 2 cap e^cap V < FLT_MAX).  Neither value is clamped at zero: rounding may leave a tiny negative number.
// rowmap[r] outside [0, Rb) writes 0, 0 and reads neither row.
// Bits: a row's sums run per lane in index order over c = tid, tid + 512, ..., then the V % 8 tail, the wave butterfly
// and the waves in order -- a function of V and the two rows' bits only, never of R, Rb, the row's place, its
// block or the other rows of the launch (blockDim is fixed at 512).
// Identical rows give exactly +0.0 twice: every p - q is +0, so every term of A and B is a zero and A = B = +0;
// S_p and S_q add the same values in the same order, so they are the same float, their logs are the same float
// and the difference is +0.  The sweep relies on it: a cell that is still its baseline reads exactly 0.
// Rows are read with 16-B loads from the row's own start (rows of odd width are misaligned, as in the sibling
// stream kernels); the V % 8 tail goes per lane.
template <int UNR>
__global__ void __launch_bounds__(512) head_shift_kernel(const uint16_t* __restrict__ logits,
                                                         const uint16_t* __restrict__ base,
                                                         const int32_t* __restrict__ rowmap, float* __restrict__ kl,
                                                         float* __restrict__ kl_rev, int R, int Rb, int V,
                                                         const uint16_t* __restrict__ tab) {
  __shared__ Slots<float> sh[4];
  extern __shared__ __attribute__((aligned(16))) uint16_t ctab_lds[];
  const uint16_t* ct = stage_ctab(tab, ctab_lds);
  const int nv = V >> 3;
  for (int r = blockIdx.x; r < R; r += gridDim.x) {
    const int b = rowmap[r];
    if (b < 0 || b >= Rb) {   // block-uniform
      if (threadIdx.x == 0) { kl[r] = 0.f; kl_rev[r] = 0.f; }
      continue;
    }
    const uint16_t* rq = logits + (size_t)r * V;
    const uint16_t* rp = base + (size_t)b * V;
    f2 sp2 = {0.f, 0.f}, sq2 = {0.f, 0.f}, a2 = {0.f, 0.f}, b2 = {0.f, 0.f};
    auto pair8 = [&](const uint4& vp, const uint4& vq) {
      float p[8], q[8];
      capped8_tab(vp, p, ct);
      capped8_tab(vq, q, ct);
#pragma unroll
      for (int j = 0; j < 8; j += 2) {
        const f2 P = {p[j], p[j + 1]}, Q = {q[j], q[j + 1]};
        const f2 yp = P * LOG2E2, yq = Q * LOG2E2;
        const f2 ep = {__builtin_amdgcn_exp2f(yp.x), __builtin_amdgcn_exp2f(yp.y)};
        const f2 eq = {__builtin_amdgcn_exp2f(yq.x), __builtin_amdgcn_exp2f(yq.y)};
        const f2 d = P - Q;
        sp2 += ep;
        sq2 += eq;
        a2 += ep * d;
        b2 -= eq * d;
      }
    };
    {
      const uint4* pp = reinterpret_cast<const uint4*>(rp);
      const uint4* pq = reinterpret_cast<const uint4*>(rq);
      const int st = blockDim.x;
      int c = threadIdx.x;
      for (; c + (UNR - 1) * st < nv; c += UNR * st) {   // 2 UNR loads in flight per lane
        uint4 vp[UNR], vq[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) { vp[u] = pp[c + u * st]; vq[u] = pq[c + u * st]; }
#pragma unroll
        for (int u = 0; u < UNR; ++u) pair8(vp[u], vq[u]);
      }
      for (; c < nv; c += st) pair8(pp[c], pq[c]);
    }
    float sp = sp2.x + sp2.y, sq = sq2.x + sq2.y, a = a2.x + a2.y, bb = b2.x + b2.y;
    for (int c = nv * 8 + threadIdx.x; c < V; c += blockDim.x) {
      const float p = capped1(rp[c], ct, 0.f, 1), q = capped1(rq[c], ct, 0.f, 1);
      const float ep = __expf(p), eq = __expf(q), d = p - q;
      sp += ep;
      sq += eq;
      a += ep * d;
      bb -= eq * d;
    }
    block_reduce(red(sp, sh[0]), red(sq, sh[1]), red(a, sh[2]), red(bb, sh[3]));
    if (threadIdx.x == 0) {
      const float dl = __logf(sp) - __logf(sq);
      kl[r] = a / sp - dl;
      kl_rev[r] = bb / sq + dl;
    }
    __syncthreads();   // sh is rewritten by the next row
  }
}

// Output movers of an edit: where the probability went.  For selected row i with r = rows[i], b = rowmap[r],
// q = c(logits[r]) and p = c(base[b]) (head_shift_kernel's capped values, through the same LDS table):
//   pass 1   S_p = sum e^p, S_q = sum e^q -- head_shift_kernel's two sums, statement for statement
//   thread 0 rp = 1 / S_p, rq = 1 / S_q, handed to the block through LDS
//   pass 2   d_v = fl(e^{q_v} rq) - fl(e^{p_v} rp) per column (never contracted into an fma), tv = 1/2 sum |d_v|,
//            and per wave the K best gainers (d > 0) and the K best losers (d < 0) in sorted lists across its lanes
//   a merge of the eight waves' lists gives up_id / up_dp (d descending, id ascending) and dn_id / dn_dp (d
//   ascending, id ascending; the negative value); unfilled slots hold -1 and +0.0
//   dp_track[i, t] = d at column ids[i, t], through the statements its column takes in pass 2 (movers_d2 in the
//   16-B body, movers_d1 in the V % 8 tail): an id that is also listed carries the same float there.  An id outside
//   [0, V) gives 0.
// rows[i] outside [0, R) or rowmap[r] outside [0, Rb) writes 0, empty lists and zeros and reads neither row.
// Bits: d_v is a pure function of (p_v, q_v, rp, rq) and of whether column v lies in the body or the tail, which V
// alone decides; S_p, S_q and tv add per lane in index order over c = tid, tid + 512, ..., then the tail, the wave
// butterfly and the waves in order, as head_shift_kernel's sums do; the lists' order (value, then id) is total, so
// neither the traversal nor the merge order can show.  A row's outputs are a function of V, K, ids[i] and the two
// rows' bits.  Identical rows: S_p and S_q are the same float, so are rp and rq and every product, every d is +0
// and so is tv; no d > 0 or d < 0 exists, so both lists stay empty.
// The losers' list keeps -d, so one ordering serves both lists; an empty entry is (0, -1), below every real one.
constexpr int HM_KMAX = 8;    // list length (ops.HEAD_MOVERS_KMAX)
constexpr int HM_TMAX = 8;    // tracked ids per row

__device__ __forceinline__ f2 movers_d2(f2 P, f2 Q, float rp, float rq) {
#pragma clang fp contract(off)
  const f2 yp = P * LOG2E2, yq = Q * LOG2E2;
  const f2 ep = {__builtin_amdgcn_exp2f(yp.x), __builtin_amdgcn_exp2f(yp.y)};
  const f2 eq = {__builtin_amdgcn_exp2f(yq.x), __builtin_amdgcn_exp2f(yq.y)};
  const f2 a = eq * f2{rq, rq};
  const f2 b = ep * f2{rp, rp};
  return a - b;
}
__device__ __forceinline__ float movers_d1(float p, float q, float rp, float rq) {
#pragma clang fp contract(off)
  const float a = __expf(q) * rq;
  const float b = __expf(p) * rp;
  return a - b;
}

// A wave's K best (value, column) pairs, entry j in lane j, sorted (value descending, column ascending); lanes from K
// on hold the empty pair (0, -1), which is below every real one.  The K-th pair is the wave's threshold, kept
// wave-uniform, so the common case costs one compare per column and the rare entry runs once for the whole wave (a
// list per lane made nearly every column a slow one: some lane of the 64 almost always had something to insert).
// offer() takes one candidate per lane and inserts those that pass, lane by lane: the position is the number of
// entries that stay ahead, the entries behind it move down one lane.
struct WaveList {
  float v;
  int i;
  float thv;
  int thi;
  __device__ __forceinline__ void clear() {
    v = 0.f;
    i = -1;
    thv = 0.f;
    thi = -1;
  }
  __device__ __forceinline__ void offer(float x, int c, int K) {
    const int lane = threadIdx.x & 63;
    unsigned long long m = __builtin_amdgcn_ballot_w64(x > thv || (x == thv && c < thi));   // x <= 0 never passes
    while (m != 0) {   // wave-uniform
      const int src = __builtin_ctzll(m);
      m &= m - 1;
      const float xs = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), src));
      const int cs = __builtin_amdgcn_readlane(c, src);
      if (!(xs > thv || (xs == thv && cs < thi))) continue;   // the threshold has risen since the ballot
      const bool ahead = lane < K && (v > xs || (v == xs && i < cs));
      const int pos = __builtin_popcountll(__builtin_amdgcn_ballot_w64(ahead));
      const float vu = __shfl_up(v, 1, 64);
      const int iu = __shfl_up(i, 1, 64);
      if (lane >= K) { v = 0.f; i = -1; }
      else if (lane > pos) { v = vu; i = iu; }
      else if (lane == pos) { v = xs; i = cs; }
      thv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), K - 1));
      thi = __builtin_amdgcn_readlane(i, K - 1);
    }
  }
};

struct HeadMovers {
  const int32_t* rowmap;   // [R]
  const int32_t* rows;     // [Rs]
  const int32_t* ids;      // [Rs, T] or nullptr (T = 0)
  float* tv;               // [Rs]
  int32_t* up_id;          // [Rs, K]
  float* up_dp;
  int32_t* dn_id;
  float* dn_dp;
  float* dp_track;         // [Rs, T]
  int R, Rb, Rs, V, K, T;
};

template <int UNR>
__global__ void __launch_bounds__(512) head_movers_kernel(const uint16_t* __restrict__ logits,
                                                          const uint16_t* __restrict__ base,
                                                          const uint16_t* __restrict__ tab, HeadMovers hm) {
  __shared__ Slots<float> sh[3];
  __shared__ float srec[2];
  __shared__ float lv[2][8][HM_KMAX];   // the waves' lists: [up / dn][wave][entry]
  __shared__ int li[2][8][HM_KMAX];
  extern __shared__ __attribute__((aligned(16))) uint16_t ctab_lds[];
  const uint16_t* ct = stage_ctab(tab, ctab_lds);
  const int V = hm.V, K = hm.K, T = hm.T;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int nv = V >> 3;
  for (int i = blockIdx.x; i < hm.Rs; i += gridDim.x) {
    const int r = hm.rows[i];
    const int b = (r >= 0 && r < hm.R) ? hm.rowmap[r] : -1;
    if (b < 0 || b >= hm.Rb) {   // block-uniform
      if (threadIdx.x == 0) {
        hm.tv[i] = 0.f;
        for (int k = 0; k < K; ++k) {
          hm.up_id[(size_t)i * K + k] = -1;
          hm.up_dp[(size_t)i * K + k] = 0.f;
          hm.dn_id[(size_t)i * K + k] = -1;
          hm.dn_dp[(size_t)i * K + k] = 0.f;
        }
        for (int t = 0; t < T; ++t) hm.dp_track[(size_t)i * T + t] = 0.f;
      }
      continue;
    }
    const uint16_t* rq_ = logits + (size_t)r * V;
    const uint16_t* rp_ = base + (size_t)b * V;
    const uint4* pp = reinterpret_cast<const uint4*>(rp_);
    const uint4* pq = reinterpret_cast<const uint4*>(rq_);
    const int st = blockDim.x;
    // ---- pass 1: the two exp-sums (head_shift_kernel's statements for sp2 / sq2, sp / sq)
    f2 sp2 = {0.f, 0.f}, sq2 = {0.f, 0.f};
    auto sum8 = [&](const uint4& vp, const uint4& vq) {
      float p[8], q[8];
      capped8_tab(vp, p, ct);
      capped8_tab(vq, q, ct);
#pragma unroll
      for (int j = 0; j < 8; j += 2) {
        const f2 P = {p[j], p[j + 1]}, Q = {q[j], q[j + 1]};
        const f2 yp = P * LOG2E2, yq = Q * LOG2E2;
        const f2 ep = {__builtin_amdgcn_exp2f(yp.x), __builtin_amdgcn_exp2f(yp.y)};
        const f2 eq = {__builtin_amdgcn_exp2f(yq.x), __builtin_amdgcn_exp2f(yq.y)};
        sp2 += ep;
        sq2 += eq;
      }
    };
    {
      int c = threadIdx.x;
      for (; c + (UNR - 1) * st < nv; c += UNR * st) {   // 2 UNR loads in flight per lane
        uint4 vp[UNR], vq[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) { vp[u] = pp[c + u * st]; vq[u] = pq[c + u * st]; }
#pragma unroll
        for (int u = 0; u < UNR; ++u) sum8(vp[u], vq[u]);
      }
      for (; c < nv; c += st) sum8(pp[c], pq[c]);
    }
    float sp = sp2.x + sp2.y, sq = sq2.x + sq2.y;
    for (int c = nv * 8 + threadIdx.x; c < V; c += blockDim.x) {
      const float p = capped1(rp_[c], ct, 0.f, 1), q = capped1(rq_[c], ct, 0.f, 1);
      sp += __expf(p);
      sq += __expf(q);
    }
    block_reduce(red(sp, sh[0]), red(sq, sh[1]));
    if (threadIdx.x == 0) {
      srec[0] = 1.0f / sp;
      srec[1] = 1.0f / sq;
    }
    __syncthreads();
    const float rp = srec[0], rq = srec[1];
    // ---- the tracked ids, one thread each
    if ((int)threadIdx.x < T) {
      const int id = hm.ids[(size_t)i * T + threadIdx.x];
      float d = 0.f;
      if (id >= 0 && id < V) {
        const float p = capped1(rp_[id], ct, 0.f, 1), q = capped1(rq_[id], ct, 0.f, 1);
        d = id < nv * 8 ? movers_d2(f2{p, p}, f2{q, q}, rp, rq).x : movers_d1(p, q, rp, rq);
      }
      hm.dp_track[(size_t)i * T + threadIdx.x] = d;
    }
    // ---- pass 2: the differences, their absolute sum and the wave's candidates.  The lists live across the lanes of a
    // wave, so every trip is run by whole waves: a lane past the row's end takes part with zeros, which add +0 to its
    // sum (no bit changes) and are never offered
    WaveList up, dn;
    up.clear();
    dn.clear();
    f2 t2 = {0.f, 0.f};
    auto diff8 = [&](const uint4& vp, const uint4& vq, int c, bool ok) {
      float p[8], q[8], d[8];
      capped8_tab(vp, p, ct);
      capped8_tab(vq, q, ct);
#pragma unroll
      for (int j = 0; j < 8; j += 2) {
        const f2 dd = movers_d2(f2{p[j], p[j + 1]}, f2{q[j], q[j + 1]}, rp, rq);
        d[j] = ok ? dd.x : 0.f;
        d[j + 1] = ok ? dd.y : 0.f;
        t2 += f2{fabsf(d[j]), fabsf(d[j + 1])};
      }
      // one test per list and vector: nothing below the wave's threshold can enter (offer decides exactly)
      const float mx = fmaxf(fmaxf(fmaxf(d[0], d[1]), fmaxf(d[2], d[3])), fmaxf(fmaxf(d[4], d[5]), fmaxf(d[6], d[7])));
      const float mn = fminf(fminf(fminf(d[0], d[1]), fminf(d[2], d[3])), fminf(fminf(d[4], d[5]), fminf(d[6], d[7])));
      if (__builtin_amdgcn_ballot_w64(mx > 0.f && mx >= up.thv) != 0) {   // wave-uniform
#pragma unroll
        for (int j = 0; j < 8; ++j) up.offer(d[j], c * 8 + j, K);
      }
      if (__builtin_amdgcn_ballot_w64(mn < 0.f && -mn >= dn.thv) != 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) dn.offer(-d[j], c * 8 + j, K);
      }
    };
    {
      // per lane the order of the plain loop (c = tid, tid + 512, ...); the trip counts are the wave's: UNR-deep while
      // the wave's last lane has all UNR vectors, then one vector at a time while its first lane has one
      int c = threadIdx.x;
      int cw = __builtin_amdgcn_readfirstlane(threadIdx.x) + 63;
      for (; cw + (UNR - 1) * st < nv; cw += UNR * st, c += UNR * st) {
        uint4 vp[UNR], vq[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) { vp[u] = pp[c + u * st]; vq[u] = pq[c + u * st]; }
#pragma unroll
        for (int u = 0; u < UNR; ++u) diff8(vp[u], vq[u], c + u * st, true);
      }
      for (; cw - 63 < nv; cw += st, c += st) {
        const bool ok = c < nv;
        const uint4 z = {0u, 0u, 0u, 0u};
        diff8(ok ? pp[c] : z, ok ? pq[c] : z, c, ok);
      }
    }
    float ts = t2.x + t2.y;
    if (wid == 0) {   // the V % 8 tail: at most 7 columns, lanes 0..6 of wave 0 (the plain loop's lanes), as a whole wave
      const int c = nv * 8 + lane;
      const bool ok = c < V;
      const float d = ok ? movers_d1(capped1(rp_[ok ? c : 0], ct, 0.f, 1), capped1(rq_[ok ? c : 0], ct, 0.f, 1), rp, rq)
                         : 0.f;
      ts += fabsf(d);
      up.offer(d, c, K);
      dn.offer(-d, c, K);
    }
    if (lane < HM_KMAX) {   // lanes from K on hold the empty pair
      lv[0][wid][lane] = up.v;
      li[0][wid][lane] = up.i;
      lv[1][wid][lane] = dn.v;
      li[1][wid][lane] = dn.i;
    }
    block_reduce(red(ts, sh[2]));   // its barrier publishes the waves' lists as well
    if (threadIdx.x == 0) hm.tv[i] = 0.5f * ts;
    // ---- wave 0 merges the waves' sorted lists: lane w holds the head of wave w's list, K rounds of arg-best over the
    // heads, the winning lane moves on to its next entry
    if (wid == 0) {
      const int nw = blockDim.x >> 6;
      int hu = 0, hd = 0;
      for (int k = 0; k < K; ++k) {
        const ArgBest mu = (lane < nw && hu < K) ? ArgBest{lv[0][lane][hu], li[0][lane][hu]} : ArgBest{0.f, -1};
        const ArgBest md = (lane < nw && hd < K) ? ArgBest{lv[1][lane][hd], li[1][lane][hd]} : ArgBest{0.f, -1};
        ArgBest bu = mu, bd = md;
        wave_reduce(bu, bd);
        if (lane == 0) {
          hm.up_id[(size_t)i * K + k] = bu.i;
          hm.up_dp[(size_t)i * K + k] = bu.v;
          hm.dn_id[(size_t)i * K + k] = bd.i;
          hm.dn_dp[(size_t)i * K + k] = bd.v > 0.f ? -bd.v : 0.f;
        }
        if (bu.i >= 0 && mu.i == bu.i) ++hu;
        if (bd.i >= 0 && md.i == bd.i) ++hd;
      }
    }
    __syncthreads();   // the slots, srec and the lists are rewritten by the next row
  }
}

// elementwise exact softcap through the compact path (ops.softcap_values; the exhaustive GPU test)
__global__ void softcap_c_kernel(const uint16_t* __restrict__ x, float* __restrict__ y, int n, CapC cc) {
  __shared__ uint16_t lt[CAPC_MAX];
  for (int i = threadIdx.x; i < cc.hi - cc.lo; i += blockDim.x) lt[i] = cc.tab[i];
  __syncthreads();
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) y[i] = capc1(x[i], lt, cc);
}

// what the host registered per (device, cap bits): the 64 KB softcap tables and the compact softcaps
template <typename P>
struct CapRegistry {
  struct Entry {
    int dev;
    uint32_t capbits;
    P p;
  };
  Entry e[16];
  int n = 0;

  // the entry of ``cap`` on the current device; with ``add`` a new one is made if there is room.  nullptr: none
  P* find(float cap, bool add = false) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint32_t cb = __builtin_bit_cast(uint32_t, cap);
    for (int i = 0; i < n; ++i)
      if (e[i].dev == dev && e[i].capbits == cb) return &e[i].p;
    if (!add || n >= 16) return nullptr;
    e[n] = Entry{dev, cb, P{}};
    return &e[n++].p;
  }
};
CapRegistry<const uint16_t*> g_tabs;
CapRegistry<CapC> g_capc;

const uint16_t* find_tab(float cap, int emulate) {
  if (!(cap > 0.f) || !emulate) return nullptr;
  const uint16_t* const* t = g_tabs.find(cap);
  return t != nullptr ? *t : nullptr;
}

int cu_count() {
  static const int ncu = [] {
    int dev = 0, n = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n > 0 ? n : 256;
  }();
  return ncu;
}

// TB_DECODE_HEAD, read once per process: "t" the per-row 64 KB-table kernel, "c" the compact-softcap kernel (A/B;
// both keep a running max), default "f": the fixed-offset kernels where the cap allows them
char dh_mode() {
  static const char mode = [] {
    const char* e = getenv("TB_DECODE_HEAD");
    return e != nullptr && (e[0] == 't' || e[0] == 'c') ? e[0] : 'f';
  }();
  return mode;
}

// Whether tb_decode_head runs the fixed-offset kernel at this cap, as the return code of the readouts that exist
// only there: 0 yes (*tab: its table), 1 no registered table or a cap outside (0, DH_FIXED_CAP], 2 TB_DECODE_HEAD
// selects the t / c kernel.  *tab is the registered table (or nullptr) in every case.
int fixed_path(float cap, const uint16_t** tab) {
  *tab = find_tab(cap, 1);
  if (*tab == nullptr || !(cap <= DH_FIXED_CAP)) return 1;
  return dh_mode() == 'f' ? 0 : 2;
}

// Launches one of the 512-thread row kernels, with the dynamic LDS of the 64 KB table where there is one: > 64 KB of
// LDS needs the opt-in, once per kernel (first call is never inside a graph capture).
template <auto Kern, typename... A>
void launch_rows(int grid, const uint16_t* tab, hipStream_t st, A... args) {
  size_t lds = 0;
  if (tab != nullptr) {
    static const hipError_t opted = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern),
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, CTAB_N * 2 + 256);
    (void)opted;
    lds = CTAB_N * 2;
  }
  hipLaunchKernelGGL(Kern, dim3(grid), dim3(512), lds, st, args...);
}

}  // namespace

void tb_register_softcap_table(float cap, const uint16_t* tab) {
  if (const uint16_t** t = g_tabs.find(cap, true)) *t = tab;
}

const uint16_t* tb_find_softcap_table(float cap) { return find_tab(cap, 1); }

bool tb_register_softcap_compact(float cap, const uint16_t* tab, int lo, int hi, float sat) {
  if (hi < lo || hi - lo > CAPC_MAX || !(cap > 0.f)) return false;
  CapC* c = g_capc.find(cap, true);
  if (c == nullptr) return false;
  *c = CapC{tab, lo, hi, sat, 1.0f / cap, cap};
  return true;
}

bool tb_softcap_compact_params(float cap, const uint16_t** tab, int* lo, int* hi, float* sat) {
  const CapC* c = g_capc.find(cap);
  if (c == nullptr) return false;
  *tab = c->tab;
  *lo = c->lo;
  *hi = c->hi;
  *sat = c->sat;
  return true;
}

bool tb_softcap_compact(const uint16_t* x, float* y, int n, float cap, hipStream_t st) {
  const CapC* c = g_capc.find(cap);
  if (c == nullptr || n <= 0) return c != nullptr;
  hipLaunchKernelGGL(softcap_c_kernel, dim3(std::min((n + 255) / 256, 4096)), dim3(256), 0, st, x, y, n, *c);
  return true;
}

bool tb_decode_head_stats(const uint16_t* logits, const int32_t* tgt, int off, float* stats, int R, int V, float cap,
                          hipStream_t st) {
  const uint16_t* tab;
  if (fixed_path(cap, &tab) == 1) return false;   // runs under TB_DECODE_HEAD=t / c as well
  if (R <= 0) return true;
  // UNR = 1: nobody has measured the stats pass at ROW_UNR
  launch_rows<decode_head_f_kernel<1>>(std::min(R, 2 * cu_count()), tab, st, logits, tgt, nullptr, nullptr, nullptr, R,
                                       V, tab, reinterpret_cast<float4*>(stats), off);
  return true;
}

void tb_decode_head(const uint16_t* logits, const int32_t* tgt, int32_t* nxt, float* nll_self, float* nll_tgt, int R,
                    int V, float cap, hipStream_t st) {
  if (R <= 0) return;
  const uint16_t* tab;
  if (fixed_path(cap, &tab) == 0)
    launch_rows<decode_head_f_kernel<ROW_UNR>>(std::min(R, 2 * cu_count()), tab, st, logits, tgt, nxt, nll_self,
                                               nll_tgt, R, V, tab, nullptr, 0);
  else if (const CapC* cc = g_capc.find(cap); cc != nullptr && dh_mode() != 't')
    launch_rows<decode_head_kernel<CapCompact>>(R, nullptr, st, logits, tgt, nxt, nll_self, nll_tgt, V,
                                                CapCompact{*cc, nullptr});
  else
    launch_rows<decode_head_kernel<CapRunEmu>>(R, tab, st, logits, tgt, nxt, nll_self, nll_tgt, V,
                                               CapRunEmu{{tab, cap, 1}});
}

// decode_head + tracked-id readout (decode_head_track_kernel).  Only where tb_decode_head runs the f kernel: returns 1
// without a registered table or for a cap outside (0, DH_FIXED_CAP], 2 under TB_DECODE_HEAD=t / c, 3 for T / n_rank
// out of range (nothing launched); 0 on success.
int tb_decode_head_track(const uint16_t* logits, const int32_t* tgt, int32_t* nxt, float* nll_self, float* nll_tgt,
                         const int32_t* track, int T, int n_rank, float* logp, int32_t* rank, const int64_t* col, int W,
                         int R, int V, float cap, hipStream_t st) {
  if (T < 1 || T > DH_TRACK_MAX || n_rank < 0 || n_rank > T || (col != nullptr && W < 1)) return 3;
  const uint16_t* tab;
  if (const int rc = fixed_path(cap, &tab); rc != 0) return rc;
  if (R <= 0) return 0;
  const int grid = std::min(R, 2 * cu_count());
  const HeadTrack tk{track, logp, rank, col, T, n_rank, W};
  auto go = [&](auto nr) {
    launch_rows<decode_head_track_kernel<decltype(nr)::value>>(grid, tab, st, logits, tgt, nxt, nll_self, nll_tgt, R, V,
                                                               tab, tk);
  };
  if (n_rank == 0) go(std::integral_constant<int, 0>{});
  else if (n_rank <= 2) go(std::integral_constant<int, 2>{});
  else if (n_rank <= 4) go(std::integral_constant<int, 4>{});
  else go(std::integral_constant<int, 8>{});
  return 0;
}

// KL(base || edit) and KL(edit || base) per row (head_shift_kernel).  Only where tb_decode_head runs the f kernel:
// returns 1 without a registered table or for a cap outside (0, DH_FIXED_CAP], 2 under TB_DECODE_HEAD=t / c, 3 for
// V < 1 or Rb < 0 (nothing launched); 0 on success.
int tb_head_shift(const uint16_t* logits, const uint16_t* base, const int32_t* rowmap, float* kl, float* kl_rev, int R,
                  int Rb, int V, float cap, hipStream_t st) {
  if (V < 1 || Rb < 0) return 3;
  const uint16_t* tab;
  if (const int rc = fixed_path(cap, &tab); rc != 0) return rc;
  if (R <= 0) return 0;
  launch_rows<head_shift_kernel<2>>(std::min(R, 2 * cu_count()), tab, st, logits, base, rowmap, kl, kl_rev, R, Rb, V,
                                    tab);
  return 0;
}

// Total variation, top-K gainers / losers and tracked differences of the selected rows (head_movers_kernel).  Only
// where tb_decode_head runs the f kernel: returns 1 without a registered table or for a cap outside (0,
// DH_FIXED_CAP], 2 under TB_DECODE_HEAD=t / c, 3 for V < 1, R or Rb < 0, K outside [1, 8] or T outside [0, 8]
// (nothing launched); 0 on success.
int tb_head_movers(const uint16_t* logits, const uint16_t* base, const int32_t* rowmap, const int32_t* rows,
                   const int32_t* ids, int T, int K, float* tv, int32_t* up_id, float* up_dp, int32_t* dn_id,
                   float* dn_dp, float* dp_track, int R, int Rb, int Rs, int V, float cap, hipStream_t st) {
  if (V < 1 || R < 0 || Rb < 0 || K < 1 || K > HM_KMAX || T < 0 || T > HM_TMAX || (T > 0 && ids == nullptr)) return 3;
  const uint16_t* tab;
  if (const int rc = fixed_path(cap, &tab); rc != 0) return rc;
  if (Rs <= 0) return 0;
  const HeadMovers hm{rowmap, rows, ids, tv, up_id, up_dp, dn_id, dn_dp, dp_track, R, Rb, Rs, V, K, T};
  launch_rows<head_movers_kernel<2>>(std::min(Rs, 2 * cu_count()), tab, st, logits, base, tab, hm);
  return 0;
}

void tb_argmax_rows(const uint16_t* logits, int32_t* out, int R, int V, float cap, hipStream_t st) {
  if (R <= 0) return;
  const uint16_t* tab = find_tab(cap, 1);
  launch_rows<argmax_rows_kernel>(R, tab, st, logits, out, V, cap, tab);
}

void tb_row_lse(const uint16_t* logits, float* lse, int R, int V, float cap, int emulate_bf16, hipStream_t st) {
  if (R <= 0) return;
  const uint16_t* tab = find_tab(cap, emulate_bf16);
  launch_rows<row_lse_kernel>(R, tab, st, logits, lse, V, cap, emulate_bf16, tab);
}

void tb_gather_probs(const uint16_t* logits, const float* lse, const int32_t* ids, float* out, int R, int K, int V,
                     int round_bf16, const int32_t* rowmap, hipStream_t st) {
  if (R <= 0 || K <= 0) return;
  const int n = R * K;
  hipLaunchKernelGGL(gather_probs_kernel, dim3((n + 255) / 256), dim3(256), 0, st, logits, lse, ids, out, R, K, V,
                     round_bf16, rowmap);
}

void tb_lens_colsum(const uint16_t* logits, const float* lse, const uint8_t* mask, const int32_t* excl, float* acc,
                    int B, int T, int V, int accumulate, int round_bf16, const int32_t* offs, float* cum,
                    const int32_t* rowmap, hipStream_t st) {
  if (B <= 0) return;
  const int groups = (V + 7) / 8;
  dim3 grid((groups + 255) / 256, B);
  hipLaunchKernelGGL(lens_colsum_kernel, grid, dim3(256), 0, st, logits, lse, mask, excl, acc, T, V, accumulate,
                     round_bf16, offs, cum, rowmap);
}

int tb_topk_chunks(int R, int V) { return (R >= 512 || V <= 4096) ? 1 : (V + 2047) / 2048; }

namespace {
void topk_launch(const float* x, const int32_t* xi, float* vals, int32_t* idx, int R, int V, int K, int CH, int C,
                 hipStream_t st) {
  const dim3 g(R * C);
  if (K <= 8) hipLaunchKernelGGL(topk_rows_kernel<8>, g, dim3(256), 0, st, x, xi, vals, idx, V, K, CH, C);
  else if (K <= 16) hipLaunchKernelGGL(topk_rows_kernel<16>, g, dim3(256), 0, st, x, xi, vals, idx, V, K, CH, C);
  else hipLaunchKernelGGL(topk_rows_kernel<64>, g, dim3(256), 0, st, x, xi, vals, idx, V, K, CH, C);
}
}  // namespace

// few long rows (the lens top-k over the vocabulary: a few hundred workgroups streaming 1 MB rows cannot fill the
// chip): C chunks of each row give C * K candidates each, then one pass over the candidates per row
void tb_topk_rows(const float* x, float* vals, int32_t* idx, int R, int V, int K, float* wv, int32_t* wi, int C,
                  hipStream_t st) {
  if (R <= 0) return;
  if (C <= 1 || wv == nullptr || wi == nullptr) {
    topk_launch(x, nullptr, vals, idx, R, V, K, V, 1, st);
    return;
  }
  const int CH = (((V + C - 1) / C) + 3) & ~3;
  topk_launch(x, nullptr, wv, wi, R, V, K, CH, C, st);
  topk_launch(wv, wi, vals, idx, R, C * K, K, C * K, 1, st);
}

void tb_xent_rows(const uint16_t* logits, const int32_t* tgt, float* nll, int R, int V, float cap, int emulate_bf16,
                  hipStream_t st) {
  if (R <= 0) return;
  const uint16_t* tab = find_tab(cap, emulate_bf16);
  launch_rows<xent_rows_kernel>(R, tab, st, logits, tgt, nll, V, cap, emulate_bf16, tab);
}
