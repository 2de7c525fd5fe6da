// Kernels of validation and the multi-view test (engines/engine_for_finetuning.py:147-295: validation_one_epoch, final_test, merge,
// compute_video):
//   * the row pass of a test batch: cross entropy and the rank of the label per logits row, accumulated into a meter block that LIVES IN
//     DEVICE MEMORY (no host read in the batch loop), and the row's logits stored into a per-(video, view) table under the reference's
//     "the first line read wins" rule (:267-268);
//   * finalize: softmax of every present view, their mean, argmax and the rank of the label -- `merge` / `compute_video` as one kernel;
//   * the ownership mask that makes the table's sum over the ranks exact.
// All memory-bound; same idiom as finetune.hip / bert.hip: 256 threads, one workgroup per logits row or per video, 16-byte accesses on aligned
// rows, fp32 math (expf / logf, not the fast variants: the results are compared with fp64 at 1e-6), ld_logits-style tails.  No float atomics:
// the only atomic is a 64-bit integer min, which commutes, so two runs over the same batches agree bit for bit.
#include "common.h"
#include "../../include/internvideo_hip.h"

namespace ivh {
namespace evaluate {

constexpr long long NO_OWNER = 0x7fffffffffffffffLL;
// meter block, eight 8-byte slots
enum { M_LOSS = 0, M_ACC1 = 1, M_ACC5 = 2, M_BATCHES = 3, M_TOP1 = 4, M_TOP5 = 5, M_SAMPLES = 6, M_BAD = 7 };

// eight values at columns base .. base + 7 of a row with V valid columns; columns >= V read as -inf and are never dereferenced
template <typename TX>
__device__ __forceinline__ void ld_logits(const TX* xr, int base, int V, bool aligned, float* v) {
  if (aligned && base + 8 <= V) {
    if constexpr (sizeof(TX) == 4) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(xr + base), b = *reinterpret_cast<const f32x4*>(xr + base + 4);
      v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
    } else {
      unpack8(*reinterpret_cast<const u32x4*>(xr + base), v);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (base + e < V) {
        if constexpr (sizeof(TX) == 4) v[e] = xr[base + e];
        else v[e] = bf2f(xr[base + e]);
      } else v[e] = -INFINITY;
    }
  }
}

__device__ __forceinline__ void online_merge(float& m, float& s, float m2, float s2) {
  const float mx = fmaxf(m, m2);
  s = (m == -INFINITY ? 0.f : s * expf(m - mx)) + (m2 == -INFINITY ? 0.f : s2 * expf(m2 - mx));
  m = mx;
}

// (max, sum exp(x - max)) of a row over the whole workgroup; every thread gets the pair.  sm / ss: 4 floats each.
template <typename TX>
__device__ __forceinline__ void row_max_sum(const TX* xr, int V, bool aligned, float* sm, float* ss, float& m, float& s) {
  const int tid = threadIdx.x, nch = (V + 7) >> 3;
  m = -INFINITY; s = 0.f;
  for (int c = tid; c < nch; c += 256) {
    float v[8];
    ld_logits(xr, c * 8, V, aligned, v);
    float cm = v[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) cm = fmaxf(cm, v[e]);
    float cs = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) cs += expf(v[e] - cm);                 // exp(-inf) = 0 at the tail
    online_merge(m, s, cm, cs);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    online_merge(m, s, m2, s2);
  }
  __syncthreads();                                                     // sm / ss may still be read from the previous call
  if ((tid & 63) == 0) { sm[tid >> 6] = m; ss[tid >> 6] = s; }
  __syncthreads();
  m = sm[0]; s = ss[0];
#pragma unroll
  for (int i = 1; i < 4; ++i) online_merge(m, s, sm[i], ss[i]);
}

__device__ __forceinline__ int block_sum_int(int v, int* si) {         // si[4]; every thread gets the sum
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) si[threadIdx.x >> 6] = v;
  __syncthreads();
  return (si[0] + si[1]) + (si[2] + si[3]);
}

__device__ __forceinline__ bool slot_ok(int vid, int vw, int n_videos, int n_views) {
  return vid >= 0 && vid < n_videos && vw >= 0 && vw < n_views;
}

// phase 1 of the view table: owner[video, view] = min(owner, seq_base + row).  A 64-bit integer min commutes: the result does not depend on
// the order in which the rows arrive.
__global__ __launch_bounds__(256) void claim_kernel(const int* __restrict__ video, const int* __restrict__ view, int M, int n_videos, int n_views,
                                                    long long seq_base, long long* __restrict__ owner) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= M) return;
  const int vid = video[row], vw = view[row];
  if (!slot_ok(vid, vw, n_videos, n_views)) return;
  atomicMin(owner + (long)vid * n_views + vw, seq_base + row);
}

// One workgroup per logits row.  loss[row] = logsumexp - x[label]; rank[row] = #{c : x_c > x_label} + #{c < label : x_c == x_label}, stored as
// ~rank (negative) for a BAD row: a label outside [0, V) (loss 0, rank V), or, with a table, video >= n_videos or view outside [0, n_views).
// A row whose sequence number is the slot's owner after the claim phase stores its logits (zeros in the slot's padding columns) and label.
template <typename TX, typename TT>
__global__ __launch_bounds__(256) void eval_rows_kernel(const TX* __restrict__ x, int ld, int V, const int* __restrict__ label,
                                                        const int* __restrict__ video, const int* __restrict__ view, long long seq_base,
                                                        int n_videos, int n_views, TT* __restrict__ table, int ldt,
                                                        const long long* __restrict__ owner, int* __restrict__ table_label,
                                                        float* __restrict__ loss, int* __restrict__ rank) {
  __shared__ float sm[4], ss[4];
  __shared__ int si[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const TX* xr = x + (long)row * ld;
  const bool aligned = (((uintptr_t)xr) & 15) == 0;
  const int lab = label[row];
  const bool lab_ok = lab >= 0 && lab < V;
  float m, s;
  row_max_sum(xr, V, aligned, sm, ss, m, s);
  float xa = -INFINITY;
  if (lab_ok) {
    if constexpr (sizeof(TX) == 4) xa = xr[lab];
    else xa = bf2f(xr[lab]);
  }
  bool bad = !lab_ok, store = false;
  long slot = 0;
  if (video) {
    const int vid = video[row], vw = view[row];
    if (vid >= 0) {                                                    // video < 0: meters only (validation_one_epoch)
      if (slot_ok(vid, vw, n_videos, n_views)) {
        slot = (long)vid * n_views + vw;
        store = lab_ok && owner[slot] == seq_base + row;
      } else bad = true;
    }
  }
  TT* tr = store ? table + slot * ldt : nullptr;
  const int nch = (V + 7) >> 3;
  int above = 0;
  for (int c = tid; c < nch; c += 256) {
    float v[8];
    const int base = c * 8;
    ld_logits(xr, base, V, aligned, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int col = base + e;
      if (col < V) above += (v[e] > xa) || (v[e] == xa && col < lab);
      else v[e] = 0.f;
    }
    if (tr) {                                                          // ldt % 8 == 0 and a 16-byte aligned table: whole chunks
      if constexpr (sizeof(TT) == 4) {
        *reinterpret_cast<f32x4*>(tr + base) = f32x4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(tr + base + 4) = f32x4{v[4], v[5], v[6], v[7]};
      } else {
        *reinterpret_cast<u32x4*>(tr + base) = pack8(v);
      }
    }
  }
  above = block_sum_int(above, si);
  if (tid == 0) {
    const int r = lab_ok ? above : V;
    loss[row] = lab_ok ? (m - xa) + logf(s) : 0.f;
    rank[row] = bad ? ~r : r;
    if (store) table_label[slot] = lab;
  }
}

// One workgroup: the batch's contribution to the meter block.  The rows' losses are summed in double in a FIXED order (thread t takes rows
// t, t + 256, ...; then a fixed tree), so the block is reproducible.  acc1 / acc5 totals are kept the way timm's `accuracy` and
// MetricLogger.update(acc.item(), n = batch) build them: fp32 (hits * 100 / batch), times batch, summed in double.
__global__ __launch_bounds__(256) void meters_kernel(const float* __restrict__ loss, const int* __restrict__ rank, int M, long long* __restrict__ meters) {
  __shared__ double sd[256];
  __shared__ int s1[256], s5[256], sb[256];
  const int tid = threadIdx.x;
  double a = 0.0;
  int h1 = 0, h5 = 0, nb = 0;
  for (int r = tid; r < M; r += 256) {
    a += (double)loss[r];
    int k = rank[r];
    if (k < 0) { k = ~k; ++nb; }
    h1 += k < 1; h5 += k < 5;
  }
  sd[tid] = a; s1[tid] = h1; s5[tid] = h5; sb[tid] = nb;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { sd[tid] += sd[tid + o]; s1[tid] += s1[tid + o]; s5[tid] += s5[tid + o]; sb[tid] += sb[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {
    double* md = reinterpret_cast<double*>(meters);
    md[M_LOSS] += sd[0] / (double)M;
    const float a1 = (float)s1[0] * 100.f / (float)M, a5 = (float)s5[0] * 100.f / (float)M;
    md[M_ACC1] += (double)a1 * (double)M;
    md[M_ACC5] += (double)a5 * (double)M;
    meters[M_BATCHES] += 1;
    meters[M_TOP1] += s1[0];
    meters[M_TOP5] += s5[0];
    meters[M_SAMPLES] += M;
    meters[M_BAD] += sb[0];
  }
}

// One workgroup per video.  acc (dynamic LDS, ldt floats): sum over the present views, ascending, of softmax(slot); column col always belongs
// to thread (col / 8) % 256 until the barrier in front of the output pass.  A slot whose owner is NO_OWNER is never read.
// out[video] = {count, pred, rank, label}: pred = first maximum of the mean, rank of the label in the mean with the tie rule above, label =
// the one stored with the lowest present view; {0, -1, -1, -1} and a zero probs row for a video without a view.
template <typename TT>
__global__ __launch_bounds__(256) void finalize_kernel(const TT* __restrict__ table, int ldt, int V, int n_views, const long long* __restrict__ owner,
                                                       const int* __restrict__ table_label, int* __restrict__ out, float* __restrict__ probs, long ldp) {
  extern __shared__ float acc[];
  __shared__ float sm[4], ss[4];
  __shared__ int si[4];
  __shared__ float bv[4];
  __shared__ int bi[4];
  const int vid = blockIdx.x, tid = threadIdx.x;
  const int nch = (V + 7) >> 3;
  for (int c = tid; c < nch; c += 256) {
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[c * 8 + e] = 0.f;
  }
  int count = 0, lab = -1;
  for (int vw = 0; vw < n_views; ++vw) {
    const long slot = (long)vid * n_views + vw;
    if (owner[slot] == NO_OWNER) continue;                             // uniform over the workgroup
    if (count == 0) lab = table_label[slot];
    ++count;
    const TT* tr = table + slot * ldt;
    float m, s;
    row_max_sum(tr, V, true, sm, ss, m, s);
    const float inv = 1.0f / s;
    for (int c = tid; c < nch; c += 256) {
      float v[8];
      ld_logits(tr, c * 8, V, true, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[c * 8 + e] += expf(v[e] - m) * inv;   // exp(-inf) = 0 at the tail
    }
  }
  __syncthreads();
  float* pr = probs ? probs + (long)vid * ldp : nullptr;
  if (count == 0) {
    if (pr) for (int col = tid; col < V; col += 256) pr[col] = 0.f;
    if (tid == 0) { out[4 * vid] = 0; out[4 * vid + 1] = -1; out[4 * vid + 2] = -1; out[4 * vid + 3] = -1; }
    return;
  }
  const float fc = (float)count;
  const bool lab_ok = lab >= 0 && lab < V;
  const float pa = lab_ok ? acc[lab] / fc : INFINITY;
  float best = -INFINITY;
  int besti = 0x7fffffff, above = 0;
  for (int col = tid; col < V; col += 256) {
    const float p = acc[col] / fc;
    if (pr) pr[col] = p;
    if (p > best) { best = p; besti = col; }                           // ascending columns per thread: the first maximum stays
    above += (p > pa) || (p == pa && col < lab);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float b2 = __shfl_xor(best, o, 64);
    const int i2 = __shfl_xor(besti, o, 64);
    if (b2 > best || (b2 == best && i2 < besti)) { best = b2; besti = i2; }
  }
  if ((tid & 63) == 0) { bv[tid >> 6] = best; bi[tid >> 6] = besti; }
  above = block_sum_int(above, si);                                    // its barriers publish bv / bi too
  if (tid == 0) {
#pragma unroll
    for (int i = 1; i < 4; ++i)
      if (bv[i] > best || (bv[i] == best && bi[i] < besti)) { best = bv[i]; besti = bi[i]; }
    out[4 * vid] = count; out[4 * vid + 1] = besti; out[4 * vid + 2] = lab_ok ? above : V; out[4 * vid + 3] = lab;
  }
}

// zero every slot (logits row and label) whose owner's rank field (owner >> 40) is not `rank`; a slot without an owner has the field of
// NO_OWNER, which no rank equals.  One wave per slot.
template <typename TT>
__global__ __launch_bounds__(256) void mask_owned_kernel(TT* __restrict__ table, int ldt, const long long* __restrict__ owner,
                                                         int* __restrict__ table_label, long n_slots, int rank) {
  const int lane = threadIdx.x & 63;
  const int nv = ldt * (int)sizeof(TT) / 16;                           // 16-byte chunks of a slot
  for (long slot = (long)blockIdx.x * 4 + (threadIdx.x >> 6); slot < n_slots; slot += (long)gridDim.x * 4) {
    if ((owner[slot] >> 40) == (long long)rank) continue;
    u32x4* tr = reinterpret_cast<u32x4*>(table + slot * ldt);
    for (int c = lane; c < nv; c += 64) tr[c] = u32x4{0u, 0u, 0u, 0u};
    if (lane == 0) table_label[slot] = 0;
  }
}

}  // namespace evaluate
}  // namespace ivh

using namespace ivh;
using namespace ivh::evaluate;

static const int FINALIZE_MAX_V = 15360;                               // 60 KiB of dynamic LDS for the mean

extern "C" int ivh_eval_rows(const void* logits, int logits_fp32, int ld, int M, int V, const int32_t* label, const int32_t* video,
                             const int32_t* view, int64_t seq_base, int n_videos, int n_views, void* table, int table_fp32, int ldt,
                             int64_t* owner, int32_t* table_label, float* loss_rows, int32_t* rank_rows, int64_t* meters, void* stream) {
  IVH_REQUIRE(logits && label && loss_rows && rank_rows && M > 0 && V > 0 && ld >= V, "eval_rows: bad args");
  IVH_REQUIRE((uintptr_t)logits % (logits_fp32 ? 4 : 2) == 0, "eval_rows: logits misaligned");
  IVH_REQUIRE(!meters || (uintptr_t)meters % 8 == 0, "eval_rows: the meter block is eight 8-byte slots, 8-byte aligned");
  if (video || view || table || owner || table_label) {
    IVH_REQUIRE(video && view && table && owner && table_label, "eval_rows: the view table needs video, view, table, owner and table_label together");
    IVH_REQUIRE(n_videos > 0 && n_views > 0, "eval_rows: n_videos = %d, n_views = %d", n_videos, n_views);
    IVH_REQUIRE(ldt >= V && ldt % 8 == 0 && (uintptr_t)table % 16 == 0, "eval_rows: the table's row pitch is a multiple of 8 >= V, its base 16-byte aligned");
    IVH_REQUIRE((uintptr_t)owner % 8 == 0, "eval_rows: owner misaligned");
    IVH_REQUIRE(seq_base >= 0 && (seq_base & ((1LL << 40) - 1)) + M <= (1LL << 40) && (seq_base >> 40) < (1LL << 22),
                "eval_rows: sequence numbers are (rank << 40) | row counter with rank < 2^22 and the counter below 2^40");
  }
  hipStream_t st = (hipStream_t)stream;
  if (video) {
    hipLaunchKernelGGL(claim_kernel, dim3((M + 255) / 256), dim3(256), 0, st, video, view, M, n_videos, n_views, (long long)seq_base, (long long*)owner);
    if (ivh_host::check_launch("eval_rows (claim)")) return -1;
  }
#define IVH_EVAL_ROWS(TX, TT)                                                                                                              \
  hipLaunchKernelGGL((eval_rows_kernel<TX, TT>), dim3(M), dim3(256), 0, st, (const TX*)logits, ld, V, label, video, view, (long long)seq_base, \
                     n_videos, n_views, (TT*)table, ldt, (const long long*)owner, table_label, loss_rows, rank_rows)
  if (logits_fp32 && table_fp32) IVH_EVAL_ROWS(float, float);
  else if (logits_fp32) IVH_EVAL_ROWS(float, bf16_t);
  else if (table_fp32) IVH_EVAL_ROWS(bf16_t, float);
  else IVH_EVAL_ROWS(bf16_t, bf16_t);
#undef IVH_EVAL_ROWS
  if (ivh_host::check_launch("eval_rows")) return -1;
  if (meters) {
    hipLaunchKernelGGL(meters_kernel, dim3(1), dim3(256), 0, st, loss_rows, rank_rows, M, (long long*)meters);
    return ivh_host::check_launch("eval_rows (meters)");
  }
  return 0;
}

extern "C" int ivh_view_finalize(const void* table, int table_fp32, int ldt, int V, int n_videos, int n_views, const int64_t* owner,
                                 const int32_t* table_label, int32_t* out, float* probs, int64_t ldp, void* stream) {
  IVH_REQUIRE(table && owner && table_label && out && V > 0 && n_videos > 0 && n_views > 0, "view_finalize: bad args");
  IVH_REQUIRE(ldt >= V && ldt % 8 == 0 && (uintptr_t)table % 16 == 0, "view_finalize: the table's row pitch is a multiple of 8 >= V, its base 16-byte aligned");
  IVH_REQUIRE(V <= FINALIZE_MAX_V, "view_finalize: V = %d exceeds %d (the mean is kept in LDS)", V, FINALIZE_MAX_V);
  IVH_REQUIRE(!probs || ldp >= V, "view_finalize: probs row pitch %ld < V", (long)ldp);
  const size_t lds = (size_t)((V + 7) / 8 * 8) * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  if (table_fp32)
    hipLaunchKernelGGL(finalize_kernel<float>, dim3(n_videos), dim3(256), lds, st, (const float*)table, ldt, V, n_views, (const long long*)owner,
                       table_label, out, probs, (long)ldp);
  else
    hipLaunchKernelGGL(finalize_kernel<bf16_t>, dim3(n_videos), dim3(256), lds, st, (const bf16_t*)table, ldt, V, n_views, (const long long*)owner,
                       table_label, out, probs, (long)ldp);
  return ivh_host::check_launch("view_finalize");
}

extern "C" int ivh_view_mask_owned(void* table, int table_fp32, int ldt, const int64_t* owner, int32_t* table_label, int64_t n_slots, int rank,
                                   void* stream) {
  IVH_REQUIRE(table && owner && table_label && n_slots > 0, "view_mask_owned: bad args");
  IVH_REQUIRE(ldt > 0 && ldt % 8 == 0 && (uintptr_t)table % 16 == 0, "view_mask_owned: the table's row pitch is a multiple of 8, its base 16-byte aligned");
  IVH_REQUIRE(rank >= 0 && rank < (1 << 22), "view_mask_owned: rank = %d outside [0, 2^22)", rank);
  const long nb = (n_slots + 3) / 4;
  hipStream_t st = (hipStream_t)stream;
  if (table_fp32)
    hipLaunchKernelGGL(mask_owned_kernel<float>, dim3((unsigned)(nb < 8192 ? nb : 8192)), dim3(256), 0, st, (float*)table, ldt, (const long long*)owner,
                       table_label, (long)n_slots, rank);
  else
    hipLaunchKernelGGL(mask_owned_kernel<bf16_t>, dim3((unsigned)(nb < 8192 ? nb : 8192)), dim3(256), 0, st, (bf16_t*)table, ldt, (const long long*)owner,
                       table_label, (long)n_slots, rank);
  return ivh_host::check_launch("view_mask_owned");
}
