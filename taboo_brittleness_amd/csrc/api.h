// Host launchers for the gfx950 kernels.  Raw pointers + stream only, so the
// .hip translation units never include the (slow to compile) torch headers;
// bindings.cpp does the tensor checks and passes the current HIP stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// norm.hip
void tb_rmsnorm(const uint16_t* x, const uint16_t* w, uint16_t* y, int M, int D, float eps, hipStream_t st);
void tb_add_rmsnorm2(uint16_t* h, const uint16_t* o, const uint16_t* w_post, const uint16_t* w_next, uint16_t* x,
                     int M, int D, float eps, hipStream_t st);
void tb_embed_rmsnorm(const int32_t* ids, const uint16_t* E, const uint16_t* w, uint16_t* h, uint16_t* x, int M,
                      int D, int V, float scale, float eps, hipStream_t st);
// rope.hip
void tb_rope_qkv_cache(const uint16_t* qkv, const int32_t* pos, const int32_t* slot_of_row, const float* cos_t,
                       const float* sin_t, uint16_t* q_out, uint16_t* kc, uint16_t* vc, int M, int Hq, int Hkv,
                       int HD, int S, int max_pos, hipStream_t st);
// the same from the ks fp32 split-K partials [ks, M, (Hq + 2 Hkv) HD] of the QKV projection (summed in order, bf16)
void tb_rope_qkv_cache_part(const float* part, int ks, const int32_t* pos, const int32_t* slot_of_row,
                            const float* cos_t, const float* sin_t, uint16_t* q_out, uint16_t* kc, uint16_t* vc, int M,
                            int Hq, int Hkv, int HD, int S, int max_pos, hipStream_t st);
void tb_kv_fanout(uint16_t* kc, uint16_t* vc, const int32_t* src_row, const int32_t* slot, const int32_t* pos, int M,
                  int nlayers, int slots, int Hkv, int S, int HD, hipStream_t st);
// attention.hip
int tb_attention_lds_bytes(int HD);
// decode row count at or below which the 4-wave-per-(row, kv head) decode kernel runs (bit-identical to the one-wave
// kernel), for rows without / with a shared prefix; n < 0: query only; returns the previous value
int tb_attention_split_rows(int n, bool prefix);
// pkc/pvc/pslot/plen (decode only, T == 1; nullptr = none): row b reads keys [0, plen[b]) from slot
// pslot[b] of the shared prefix cache (pkc, pvc) [P, Hkv, S, HD] instead of its own slot.
void tb_attention(const uint16_t* q, const uint16_t* kc, const uint16_t* vc, uint16_t* out, const int32_t* pos,
                  const int32_t* slot, int B, int T, int Hq, int Hkv, int HD, int S, float scale, float softcap,
                  int window, hipStream_t st, const uint16_t* pkc = nullptr, const uint16_t* pvc = nullptr,
                  const int32_t* pslot = nullptr, const int32_t* plen = nullptr);
// blk [nblk, bw]: (first row, rows, slot) (bw = 3) or + (prefix slot, prefix length) (bw = 5, keys below the
// prefix length read from that slot of pkc/pvc).
void tb_attention_varlen(const uint16_t* q, const uint16_t* kc, const uint16_t* vc, uint16_t* out, const int32_t* pos,
                         const int32_t* blk, int nblk, int Hq, int Hkv, int HD, int S, float scale, float softcap,
                         int window, hipStream_t st, int bw = 3, const uint16_t* pkc = nullptr,
                         const uint16_t* pvc = nullptr);
// elementwise.hip
void tb_geglu(const uint16_t* gu, uint16_t* out, int M, int F, hipStream_t st);
// lens.hip
void tb_argmax_rows(const uint16_t* logits, int32_t* out, int R, int V, float cap, hipStream_t st);
void tb_row_lse(const uint16_t* logits, float* lse, int R, int V, float cap, int emulate_bf16, hipStream_t st);
void tb_gather_probs(const uint16_t* logits, const float* lse, const int32_t* ids, float* out, int R, int K, int V,
                     int round_bf16, const int32_t* rowmap, hipStream_t st);
void tb_lens_colsum(const uint16_t* logits, const float* lse, const uint8_t* mask, const int32_t* excl, float* acc,
                    int B, int T, int V, int accumulate, int round_bf16, const int32_t* offs, float* cum,
                    const int32_t* rowmap, hipStream_t st);
// (chunked when C > 1: workspaces wv / wi of R * C * K entries; C from tb_topk_chunks)
int tb_topk_chunks(int R, int V);
void tb_topk_rows(const float* x, float* vals, int32_t* idx, int R, int V, int K, float* wv, int32_t* wi, int C,
                  hipStream_t st);
void tb_xent_rows(const uint16_t* logits, const int32_t* tgt, float* nll, int R, int V, float cap, int emulate_bf16,
                  hipStream_t st);
void tb_register_softcap_table(float cap, const uint16_t* tab);   // [32768] bf16 softcap of +bf16 bit patterns
void tb_decode_head(const uint16_t* logits, const int32_t* tgt, int32_t* nxt, float* nll_self, float* nll_tgt, int R,
                    int V, float cap, hipStream_t st);
// vocab-parallel head: per row {lse, best, best id + off, target logit or -inf} (float4) of this rank's V columns;
// false when the cap has no registered table (caller falls back)
bool tb_decode_head_stats(const uint16_t* logits, const int32_t* tgt, int off, float* stats, int R, int V, float cap,
                          hipStream_t st);
// decode_head plus, per row, the log-prob (capped logit - lse) of T <= 8 tracked vocab ids ([R, T] int32, -1 = empty)
// and the rank (count of strictly greater capped logits) of the first n_rank of them.  logp / rank are [R, T], or with
// col ([R] int64) [R, W, T] written at column min(col[r], W - 1).  0 = launched; 1 = no softcap table / cap outside
// the f kernel's range; 2 = TB_DECODE_HEAD selects another kernel; 3 = T / n_rank / W out of range.
int tb_decode_head_track(const uint16_t* logits, const int32_t* tgt, int32_t* nxt, float* nll_self, float* nll_tgt,
                         const int32_t* track, int T, int n_rank, float* logp, int32_t* rank, const int64_t* col, int W,
                         int R, int V, float cap, hipStream_t st);
// output shift: for row r and b = rowmap[r] ([R] int32), kl[r] = KL(softmax c(base[b]) || softmax c(logits[r])) and
// kl_rev[r] the reverse, on the capped logits of tb_decode_head's f kernel; rowmap[r] outside [0, Rb) writes 0, 0.
// Return codes as tb_decode_head_track (3 = V < 1).
int tb_head_shift(const uint16_t* logits, const uint16_t* base, const int32_t* rowmap, float* kl, float* kl_rev, int R,
                  int Rb, int V, float cap, hipStream_t st);
// output movers: for selected row i with r = rows[i] ([Rs] int32) and b = rowmap[r], d = softmax c(logits[r]) -
// softmax c(base[b]): tv[i] = 1/2 sum |d|, up_id / up_dp [Rs, K] the K largest d > 0 (d descending, id ascending),
// dn_id / dn_dp [Rs, K] the K smallest d < 0 (d ascending, id ascending), unfilled slots -1 / +0.0, dp_track [Rs, T] =
// d at ids [Rs, T] (0 for an id outside [0, V)).  rows[i] outside [0, R) or rowmap[r] outside [0, Rb) writes zeros and
// empty lists.  Return codes as tb_decode_head_track (3 = V < 1, K outside [1, 8] or T outside [0, 8]).
int tb_head_movers(const uint16_t* logits, const uint16_t* base, const int32_t* rowmap, const int32_t* rows,
                   const int32_t* ids, int T, int K, float* tv, int32_t* up_id, float* up_dp, int32_t* dn_id,
                   float* dn_dp, float* dp_track, int R, int Rb, int Rs, int V, float cap, hipStream_t st);
// sae.hip
void tb_head_merge(const float* part, int npart, const int32_t* tgt, const float* tgt_logit, int32_t* nxt,
                   float* nll_self, float* nll_tgt, float* lse, int M, int V, hipStream_t st);
void tb_head_fused4(const uint16_t* A, const uint16_t* W, float* part, float cap, const int32_t* tgt,
                    float* tgt_logit, int32_t* nxt, float* nll_self, float* nll_tgt, int M, int N, int K, hipStream_t st);
// cs: the RoPE table as bf16 (cos, sin) pairs [max_pos, 128, 2] (the fp32 tables rounded once: the epilogue rounds
// them to bf16 anyway, rope.hip's chain)
// a2 / k0 (multi-adapter LoRA): the GEMM's A operand is [A (k0 columns) | a2 (K - k0 columns)] (two sources, no copy)
void tb_gemm4_qkv_rope(const uint16_t* A, const uint16_t* W, const int32_t* pos, const int32_t* slot_of_row,
                       const uint16_t* cs, uint16_t* q_out, uint16_t* kc, uint16_t* vc, int M, int K,
                       int Hq, int Hkv, int S, int max_pos, int tile_rows, hipStream_t st, const uint16_t* a2 = nullptr,
                       int k0 = 0);
bool tb_register_softcap_compact(float cap, const uint16_t* tab, int lo, int hi, float sat);
bool tb_softcap_compact(const uint16_t* x, float* y, int n, float cap, hipStream_t st);
bool tb_gemm4_ok(int M, int N, int K);
// 1 (default): the 256-row tile runs a workgroup's output tiles as one K-tile stream; 0: the plain tile loop (same
// bits, kept for A/B and the equality test).  Returns the previous setting.
int tb_gemm4_set_pipe(int on);
int tb_gemm4_splitk_ks(int M, int N, int K, int tile_rows);
int tb_gemm4_splitk_part(const uint16_t* A, const uint16_t* W, float* ws, int M, int N, int K, int tile_rows, int ks,
                         hipStream_t st);
void tb_add_rmsnorm2_part(uint16_t* h, const float* part, int ks, const uint16_t* w_post, const uint16_t* w_next,
                          uint16_t* x, int M, int D, float eps, hipStream_t st);
void tb_gemm4_splitk(const uint16_t* A, const uint16_t* W, uint16_t* out, float* ws, int M, int N, int K, int ldo,
                     int epi, int tile_rows, int ks, hipStream_t st);
// out[b] = sum_t coef[b, t] * (fp32 row at device address ptr[b, t]), V % 4 == 0 (elementwise.hip)
void tb_row_combine(const int64_t* ptr, const float* coef, float* out, int B, int T, int V, hipStream_t st);
bool tb_random_basis_ok(int D);
void tb_random_basis(const uint64_t* seeds, const int32_t* ranks, const int64_t* rows, int n, int D, float* table,
                     hipStream_t st, int qu = 1);
void tb_gemm4(const uint16_t* A, const uint16_t* W, void* C, const float* bias, const float* thr, int M, int N, int K,
              int ldc, int epi, int tile_rows, hipStream_t st, const uint16_t* a2 = nullptr, int k0 = 0);
void tb_gemm_nt(const uint16_t* A, const uint16_t* W, void* C, const float* bias, const float* thr, int M, int N,
                int K, int ldc, int epi, hipStream_t st);
// val [M, mmax] fp32 (optional): latent_affine_edit, h += sum_j (val_j - alpha a_j) D_j; null: lowrank_edit
void tb_lowrank_edit(uint16_t* h, uint16_t* x_next, const uint8_t* apply, const int32_t* idx, const int32_t* cnt,
                     int mmax, const void* E, const void* Dm, int table_f32, const float* bias, const float* thr,
                     const float* pre_bias, float alpha, const uint16_t* w_next, float eps, int M, int D,
                     float* coef_out, hipStream_t st, const float* val = nullptr);
// interchange_edit (the same kernel family): c_j = fl32(alpha a_j(h)) - fl32(alpha a_j(donor[src[row]])), donor
// [n_donor, D] bf16, src [M] int32 (outside [0, n_donor): row untouched); coef_out / dcoef_out (optional) = a_j(h) /
// a_j(donor row)
void tb_interchange_edit(uint16_t* h, uint16_t* x_next, const uint8_t* apply, const int32_t* idx, const int32_t* cnt,
                         int mmax, const void* E, const void* Dm, int table_f32, const float* bias, const float* thr,
                         const float* pre_bias, float alpha, const uint16_t* w_next, float eps, int M, int D,
                         float* coef_out, const uint16_t* donor, const int32_t* src, int n_donor, float* dcoef_out,
                         hipStream_t st);
// matched_noise.hip: the norm-matched control of lowrank_edit (val null) / latent_affine_edit: the rows they would
// edit move by n = |sum_j c_j Dm[idx_j]|_2 along z / |z|_2, z_d = rb_gauss(seeds[row], pos[row], d); rows they leave
// alone stay bit-identical.  norm_out [M] (optional) = n, 0 on the untouched rows.
void tb_matched_noise_edit(uint16_t* h, uint16_t* x_next, const uint8_t* apply, const int32_t* idx,
                           const int32_t* cnt, int mmax, const void* E, const void* Dm, int table_f32,
                           const float* bias, const float* thr, const float* pre_bias, float alpha,
                           const uint16_t* w_next, float eps, int M, int D, float* coef_out, const float* val,
                           const uint64_t* seeds, const int32_t* pos, float* norm_out, hipStream_t st);
// reconstruct-mode splice: flagged rows h <- bf16(b_dec + sum_{a_j != 0, ascending j} s_j a_j W_dec[j]) with
// a = acts[src_row[row]] (src_row null: acts[row]; out of [0, n_act_rows): row untouched), x_next = RMSNorm(h)
void tb_sae_splice_edit(uint16_t* h, uint16_t* x_next, const uint8_t* apply, const int32_t* src_row,
                        const float* acts, int n_act_rows, int L, const int32_t* idx, const int32_t* cnt, int mmax,
                        const void* Wdec, int table_f32, const float* b_dec, float alpha, const uint16_t* w_next,
                        float eps, int M, int D, hipStream_t st);
// rows[cap]: ascending indices of the set flags, -1 padded; inv[n] (optional): list position per row or -1
void tb_flag_compact(const uint8_t* flags, int n, int32_t* rows, int cap, int32_t* inv, hipStream_t st);
void tb_sae_decode_sparse(const float* acts, const void* Wdec, int table_f32, const float* b_dec, uint16_t* out_bf16,
                          float* out_f32, int M, int L, int D, hipStream_t st);
void tb_latent_score(const float* acts, const float* p, const uint8_t* spike, const int32_t* seg, float* out,
                     float* spike_mean, float* corr, int G, int L, hipStream_t st);
// latent_effect.hip: causal latent scores at R spike rows.  eff [R, L] is written in full (0 where acts <= 0) and is
// required (the segment mean reads it); score [G, L] (optional) = per-segment row mean.  mode 0: exact change of
// the softcapped lens logit under the single-latent ablation x - alpha a_j W_dec[j]; mode 1: alpha a_j (v . W_dec[j]).
// V is one row (v_per_row = 0) or one row per spike row.
void tb_latent_effect(const float* acts, const uint16_t* X, const float* V, int v_per_row, const void* Wdec,
                      int table_f32, const int32_t* seg, float* score, float* eff, int R, int G, int L, int D,
                      double alpha, double eps, double cap, int mode, hipStream_t st);
// lens_track.hip: out[r, t] = f((h_r . V[vrow[r], t]) / sqrt(|h_r|^2 / D + eps)) for h [M, D] bf16, V [U, T, D] fp32,
// vrow [M] int32 (outside [0, U): the row's T outputs are 0.0 and no table row is read), f the softcap (cap <= 0:
// identity); latent_effect's mode-0 numerics, batch-invariant.  0 = launched; 3 = T / D out of range.
int tb_lens_track(const uint16_t* h, const float* V, const int32_t* vrow, float* out, int M, int U, int T, int D,
                  double eps, double cap, hipStream_t st);
// comp_trace.hip: out[i, t, s] = (sum over segment s of X[rows[i], k] W[blk[i], t, k]) / rho_i for X [M, K] bf16,
// W [U, T, K] fp32, rows / blk [Ms] int32, S equal segments of K; rho_i = sqrt(|R[rows[i]]|^2 / Dn + eps) for
// R [M, Dn] bf16 (null: 1), also written to rms[i].  rows[i] outside [0, M) or blk[i] outside [0, U): zeros and
// rms[i] = 0, nothing read.  Batch-invariant.  0 = launched; 3 = T / S / K / Dn out of range.
int tb_seg_dots(const uint16_t* X, const float* W, const int32_t* rows, const int32_t* blk, const uint16_t* R,
                float* out, float* rms, int M, int U, int Ms, int T, int K, int S, int Dn, double eps,
                hipStream_t st);
// p2p.hip
int tb_p2p_header_bytes();
int tb_p2p_max_ranks();
void* tb_p2p_alloc(size_t bytes, int uncached);
int tb_p2p_free(void* p);
int tb_p2p_get_handle(void* p, void* handle_out);
int tb_p2p_handle_size();
void* tb_p2p_open_handle(const void* handle);
int tb_p2p_close_handle(void* p);
int tb_p2p_allreduce(void* const* bases, int rank, int world, const void* in, void* out, size_t nbytes, int is_bf16,
                     int blocks, int spin_max, int barriers, hipStream_t st);
uint32_t tb_p2p_read_error(void* own_base);

// vp.hip: vocab-parallel merges (TP head / lens)
void tb_vp_head_merge(const float* st, int tp, int R, const int32_t* tgt, int V, int32_t* nxt, float* nll_self,
                      float* nll_tgt, hipStream_t stream);
void tb_vp_lse_merge(const float* lse, int tp, int R, float* out, hipStream_t stream);
void tb_vp_topk_merge(const float* vals, const int32_t* ids, int tp, int n, int k, float* ov, int32_t* oi,
                      hipStream_t stream);
int tb_p2p_allgather(void* const* bases, int rank, int world, const void* in, void* out, size_t nbytes, int blocks,
                     int spin_max, int barriers, hipStream_t st);
void tb_slot_copy(uint16_t* dst, const uint16_t* src, const int32_t* dslot, const int32_t* sslot, int n, int nl,
                  int64_t inner, int dst_slots, int src_slots, int dst_l0, int src_l0, hipStream_t st);
void tb_lens_gemm4(const uint16_t* A, const uint16_t* W, uint16_t* logits, float* part, float* lse, int M, int N,
                   int K, hipStream_t st);
// the compact exact softcap registered for `cap` on this device (csrc/lens.hip CapC): table of [lo, hi), saturation
bool tb_softcap_compact_params(float cap, const uint16_t** tab, int* lo, int* hi, float* sat);

// decode_step.hip: per-step bookkeeping of the batched greedy decode (runtime/generation.py)
void tb_decode_pre(const int64_t* step_idx, const int32_t* tf_tgt, int32_t* tf_step, int nb, int W, hipStream_t st);
void tb_decode_post(const int32_t* nxt, const float* nll, const float* tf_nll, uint8_t* done, int64_t* step_idx,
                    int32_t* out_tok, float* out_nll, float* out_tf_nll, const int32_t* stop, int nstop, int32_t* tok,
                    int32_t* pos, int nb, int W, int pad, hipStream_t st);
void tb_share_lo_gather(const int64_t* rep, const int64_t* U, const int32_t* tok, const int32_t* pos,
                        const int32_t* slot, int32_t* s_tok, int32_t* s_pos, int32_t* s_slot, const int32_t* kp_slot,
                        const int32_t* kp_len_lo, int32_t* l_slot, int32_t* l_len_lo, int nb, int B, int S,
                        hipStream_t st);
void tb_capture_rows(uint16_t* store, const uint16_t* h, const int32_t* pos, const int32_t* slot, int n, int T, int S1,
                     int D, hipStream_t st);
void tb_row_gather(uint16_t* out, const uint16_t* src, const void* idx, bool idx64, int n, int D, hipStream_t st);
int tb_share_group_max_rows();
void tb_share_group(int64_t* gid, const int32_t* tok, int64_t* rep, int64_t* grp, int32_t* src, int64_t* U, int nb,
                    int act, int first, int64_t V, hipStream_t st);

// gemm_ring.hip: batch-invariant narrow-tile GEMM (decode / mid row counts); epi 0 bf16, 3 GeGLU (interleaved gate|up)
bool tb_gemm_ring_ok(int M, int N, int K, int epi, int bm, int bn, int var);
int tb_gemm_ring_tiles(int epi, int* bm, int* bn, int cap);
void tb_gemm_ring(const uint16_t* A, const uint16_t* W, uint16_t* C, int M, int N, int K, int ldc, int epi, int bm,
                  int bn, int var, hipStream_t st, const uint16_t* a2 = nullptr, int k0 = 0);
void tb_gemm_ring_qkv_rope(const uint16_t* A, const uint16_t* W, const int32_t* pos, const int32_t* slot_of_row,
                           const uint16_t* cs, uint16_t* q_out, uint16_t* kc, uint16_t* vc, int M,
                           int K, int Hq, int Hkv, int S, int max_pos, int bm, int bn, int var, hipStream_t st,
                           const uint16_t* a2 = nullptr, int k0 = 0);
// multi-adapter LoRA down-projection: T[m, c] = bf16(x[m] . A_all[c]) where column c belongs to the row's adapter
// (c < nsr and (c % nr) / r == adapter[m]), else 0; T is [M, N] (N = A_all rows, the padded LoRA width)
// (K chunked, batch-invariant at every M; part != nullptr: one workgroup per (tile, chunk), fp32 chunk sums in part
// [tb_lora_t_chunks(K), M, N] folded by a second kernel -- the same bits as part == nullptr)
bool tb_lora_t_ok(int M, int N, int K, int bm, int bn);
int tb_lora_t_chunks(int K);
void tb_lora_t(const uint16_t* x, const uint16_t* a_all, uint16_t* t, const int32_t* adapter, int M, int N, int K,
               int nsr, int nr, int r, int bm, int bn, hipStream_t st, int ldt = 0, float* part = nullptr);
