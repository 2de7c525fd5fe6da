// Stage-2 zero-shot retrieval evaluation: the device work between feature extraction and the metrics
// (reference InternVideo2/multi_modality/tasks/retrieval_utils.py:366-613 `evaluation`, :1243-1303 `itm_eval`).
//   ivh_topk_rows_f32        `sims.topk(k)` of every row of the similarity matrix, either direction (:398, :503)
//   ivh_softmax_axis_f32     `.softmax(dim=1)`, `.T.softmax(dim=1)`, `s * s.softmax(dim=0)`, `s.T * s.T.softmax(dim=0)` (:585-589, :598-612)
//   ivh_rerank_lists         the (video, text) pairs both top-k lists ask for, grouped by video in CSR form, each pair once
//   ivh_scatter_pair_scores  `i2t_scores_x[i, topk_idx] = score`, `t2i_scores_x[j, topk_idx] = score` (:483, :566) from the grouped scores
//   ivh_retrieval_ranks      position of the best ground-truth column in every row's descending order (:1245-1280)
// Matrices are fp32 and come with a row and a column stride in elements: the transposed direction reads the same buffer.
// All of it is latency-bound bookkeeping on ~1000 x 1000 matrices: one 256-thread workgroup per row, everything else stays in L2.
#include "common.h"
#include "../../include/internvideo_hip.h"

namespace ivh {

// fp32 -> uint32 whose unsigned order is the float order; -0.0 and +0.0 share a key (x + 0.0f is +0.0 for both zeros)
__device__ __forceinline__ unsigned topk_key(float x) {
  const unsigned b = __float_as_uint(x + 0.0f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// exclusive rank of this thread among the threads of the workgroup whose `pred` holds, in thread order, and their number (`total`).
// wcnt: 4 ints of LDS.  Holds two barriers: every thread of the workgroup must call it.
__device__ __forceinline__ int block_rank(bool pred, int* wcnt, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(pred);
  const int before = __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();                                   // the previous call's readers are done with wcnt
  if (lane == 0) wcnt[wave] = __popcll(m);
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) { const int c = wcnt[w]; base += w < wave ? c : 0; tot += c; }
  total = tot;
  return base + before;
}

// One workgroup per row.  8-bit radix select (4 rounds over a 256-bin LDS histogram) finds the k-th largest key T and the number of
// elements equal to T that belong to the answer; an ordered pass collects the elements above T and the first of those ties by column;
// a bitonic sort on (key, ~column) puts them in descending order with ties by ascending column.
__global__ __launch_bounds__(256) void topk_rows_kernel(const float* __restrict__ in, int n_cols, long rs, long cs, int k,
                                                        float* __restrict__ out_val, int* __restrict__ out_idx) {
  __shared__ int hist[256];
  __shared__ int sfx[256];
  __shared__ unsigned long long surv[1024];
  __shared__ int wcnt[4];
  __shared__ unsigned s_prefix;
  __shared__ int s_krem;
  const int tid = threadIdx.x;
  const float* row = in + (long)blockIdx.x * rs;
  if (tid == 0) { s_prefix = 0u; s_krem = k; }
  __syncthreads();
  for (int round = 0; round < 4; ++round) {
    const int shift = 24 - 8 * round;
    const unsigned himask = round == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
    const unsigned prefix = s_prefix;
    const int krem = s_krem;
    hist[tid] = 0;
    __syncthreads();
    for (int c = tid; c < n_cols; c += 256) {
      const unsigned key = topk_key(row[(long)c * cs]);
      if ((key & himask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
    }
    __syncthreads();
    // sfx[d] = number of candidates whose digit is >= d
    int v = hist[tid];
    sfx[tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const int add = tid + off < 256 ? sfx[tid + off] : 0;
      __syncthreads();
      v += add;
      sfx[tid] = v;
      __syncthreads();
    }
    const int above = tid < 255 ? sfx[tid + 1] : 0;
    if (v >= krem && above < krem) {                 // exactly one digit: the candidates' count is >= krem by construction
      s_prefix = prefix | ((unsigned)tid << shift);
      s_krem = krem - above;
    }
    __syncthreads();
  }
  const unsigned T = s_prefix;
  const int n_ties = s_krem;                         // 1 <= n_ties: elements equal to T that are admitted, lowest columns first
  const int n_gt = k - n_ties;
  int k2 = 1;
  while (k2 < k) k2 <<= 1;
  for (int i = tid; i < k2; i += 256) surv[i] = 0ull;          // padding sorts last (key 0 belongs to no non-NaN float)
  int gt_base = 0, eq_base = 0;
  for (int c0 = 0; c0 < n_cols; c0 += 256) {
    const int c = c0 + tid;
    unsigned key = 0u;
    bool gt = false, eq = false;
    if (c < n_cols) {
      key = topk_key(row[(long)c * cs]);
      gt = key > T; eq = key == T;
    }
    int tot_gt, tot_eq;
    const int rg = gt_base + block_rank(gt, wcnt, tot_gt);
    const int re = eq_base + block_rank(eq, wcnt, tot_eq);
    const unsigned long long item = ((unsigned long long)key << 32) | (unsigned)(~(unsigned)c);
    if (gt && rg < n_gt) surv[rg] = item;                      // rg < n_gt always holds; the guard keeps the store inside surv
    if (eq && re < n_ties) surv[n_gt + re] = item;
    gt_base += tot_gt; eq_base += tot_eq;
  }
  __syncthreads();
  for (int size = 2; size <= k2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (k2 >> 1); t += 256) {
        const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
        const int hi = lo | stride;
        const bool desc = (lo & size) == 0;
        const unsigned long long a = surv[lo], b = surv[hi];
        if (desc ? a < b : a > b) { surv[lo] = b; surv[hi] = a; }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < k; i += 256) {
    const int c = (int)(~(unsigned)(surv[i] & 0xFFFFFFFFull));
    const bool ok = c >= 0 && c < n_cols;                      // false only for NaN input (unspecified): keep the read inside the row
    out_idx[(long)blockIdx.x * k + i] = ok ? c : 0;
    out_val[(long)blockIdx.x * k + i] = row[(long)(ok ? c : 0) * cs];
  }
}

__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ int block_sum_int(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// out[r, c] = softmax_c(in[r, :])[c] (* in[r, c]).  One workgroup per row: max, sum of exp, quotient.
__global__ __launch_bounds__(256) void softmax_axis_kernel(const float* __restrict__ in, int n_cols, long irs, long ics,
                                                           float* __restrict__ out, long ors, long ocs, int mul_input) {
  __shared__ float red[4];
  const float* row = in + (long)blockIdx.x * irs;
  float* orow = out + (long)blockIdx.x * ors;
  float mx = -INFINITY;
  for (int c = threadIdx.x; c < n_cols; c += 256) mx = fmaxf(mx, row[(long)c * ics]);
  mx = block_max(mx, red);
  float s = 0.f;
  for (int c = threadIdx.x; c < n_cols; c += 256) s += expf(row[(long)c * ics] - mx);
  s = block_sum(s, red);
  for (int c = threadIdx.x; c < n_cols; c += 256) {
    const float x = row[(long)c * ics];
    const float p = expf(x - mx) / s;
    orow[(long)c * ocs] = mul_input ? x * p : p;
  }
}

// ---- rerank lists: a byte per (owned video, text) pair collects the two "chosen by" bits, then every video's row is compacted ----------
__global__ __launch_bounds__(256) void rerank_mark_kernel(const int* __restrict__ idx_v2t, int kv, const int* __restrict__ idx_t2v, int nt,
                                                          int kt, int v_begin, int v_end, unsigned* __restrict__ pairs) {
  const long n1 = (long)(v_end - v_begin) * kv, n2 = (long)nt * kt;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n1 + n2; e += (long)gridDim.x * 256) {
    long i, j;
    unsigned bit;
    if (e < n1) { i = v_begin + e / kv; j = idx_v2t[(long)i * kv + e % kv]; bit = 1u; }
    else { j = (e - n1) / kt; i = idx_t2v[e - n1]; bit = 2u; }
    if (i < v_begin || i >= v_end || j < 0 || j >= nt) continue;        // another rank's video, or an index outside the matrix
    const long off = (i - v_begin) * nt + j;
    atomicOr(&pairs[off >> 2], bit << (8 * (off & 3)));
  }
}

__global__ __launch_bounds__(256) void rerank_count_kernel(const unsigned char* __restrict__ pairs, int nt, int* __restrict__ counts) {
  __shared__ int red[4];
  const unsigned char* row = pairs + (long)blockIdx.x * nt;
  int n = 0;
  for (int j = threadIdx.x; j < nt; j += 256) n += row[j] != 0;
  n = block_sum_int(n, red);
  if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

// ptr[0] = 0, ptr[i + 1] = ptr[i] + counts[i]: one workgroup walks the videos 256 at a time
__global__ __launch_bounds__(256) void rerank_scan_kernel(const int* __restrict__ counts, int n, int* __restrict__ ptr) {
  __shared__ int buf[256];
  __shared__ int carry;
  if (threadIdx.x == 0) { carry = 0; ptr[0] = 0; }
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + threadIdx.x;
    int v = i < n ? counts[i] : 0;
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const int add = threadIdx.x >= off ? buf[threadIdx.x - off] : 0;
      __syncthreads();
      v += add;
      buf[threadIdx.x] = v;
      __syncthreads();
    }
    const int base = carry;
    if (i < n) ptr[i + 1] = base + v;
    __syncthreads();
    if (threadIdx.x == 255) carry = base + v;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void rerank_fill_kernel(const unsigned char* __restrict__ pairs, int nt, const int* __restrict__ ptr,
                                                          long capacity, int* __restrict__ cand, unsigned char* __restrict__ flags) {
  __shared__ int wcnt[4];
  const unsigned char* row = pairs + (long)blockIdx.x * nt;
  long pos = ptr[blockIdx.x];
  for (int j0 = 0; j0 < nt; j0 += 256) {
    const int j = j0 + threadIdx.x;
    const unsigned char f = j < nt ? row[j] : 0;
    int tot;
    const long at = pos + block_rank(f != 0, wcnt, tot);
    if (f != 0 && at >= 0 && at < capacity) { cand[at] = j; flags[at] = f; }
    pos += tot;
  }
}

__global__ __launch_bounds__(256) void scatter_pair_scores_kernel(const int* __restrict__ ptr, const int* __restrict__ cand,
                                                                  const unsigned char* __restrict__ flags, const float* __restrict__ scores,
                                                                  long capacity, int v_begin, int nt, float* __restrict__ x_v2t, long vrs,
                                                                  long vcs, float* __restrict__ x_t2v, long trs, long tcs) {
  const long i = v_begin + (long)blockIdx.x;
  long lo = ptr[blockIdx.x], hi = ptr[blockIdx.x + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > capacity ? capacity : hi;
  for (long e = lo + threadIdx.x; e < hi; e += 256) {
    const int j = cand[e];
    if (j < 0 || j >= nt) continue;
    const unsigned char f = flags[e];
    const float s = scores[e];
    if (f & 1) x_v2t[i * vrs + (long)j * vcs] = s;
    if (f & 2) x_t2v[(long)j * trs + i * tcs] = s;
  }
}

// rank[r] = min over the row's ground-truth columns g of  #{c : x[r,c] > x[r,g]} + #{c < g : x[r,c] == x[r,g]}
__global__ __launch_bounds__(256) void retrieval_ranks_kernel(const float* __restrict__ x, int n_cols, long rs, long cs,
                                                              const int* __restrict__ gt_ptr, const int* __restrict__ gt_idx,
                                                              int* __restrict__ rank) {
  __shared__ int red[4];
  const float* row = x + (long)blockIdx.x * rs;
  const long lo = gt_ptr[blockIdx.x], hi = gt_ptr[blockIdx.x + 1];
  int best = n_cols;                                  // a row without a ground truth inside the matrix ranks past the end
  for (long e = lo; e < hi; ++e) {
    const int g = gt_idx[e];
    if (g < 0 || g >= n_cols) continue;               // uniform over the workgroup: every thread reads the same g
    const float s = row[(long)g * cs];
    int n = 0;
    for (int c = threadIdx.x; c < n_cols; c += 256) {
      const float v = row[(long)c * cs];
      n += (v > s) || (v == s && c < g);
    }
    n = block_sum_int(n, red);
    best = n < best ? n : best;
  }
  if (threadIdx.x == 0) rank[blockIdx.x] = best;
}

}  // namespace ivh

using namespace ivh;

static bool fits_i32(int64_t v) { return v >= 0 && v <= 0x7FFFFFFF; }

extern "C" int ivh_topk_rows_f32(const float* in, int n_rows, int n_cols, int64_t row_stride, int64_t col_stride, int k, float* out_val,
                                 int32_t* out_idx, void* stream) {
  IVH_REQUIRE(in && out_val && out_idx, "topk_rows: null pointer");
  IVH_REQUIRE(n_rows >= 1 && n_cols >= 1, "topk_rows: empty matrix (%d x %d)", n_rows, n_cols);
  IVH_REQUIRE(row_stride >= 0 && col_stride >= 0, "topk_rows: negative stride");
  IVH_REQUIRE(k >= 1 && k <= n_cols && k <= 1024, "topk_rows: k = %d outside 1 .. min(n_cols = %d, 1024)", k, n_cols);
  hipLaunchKernelGGL(topk_rows_kernel, dim3(n_rows), dim3(256), 0, (hipStream_t)stream, in, n_cols, (long)row_stride, (long)col_stride, k,
                     out_val, out_idx);
  return ivh_host::check_launch("topk_rows");
}

extern "C" int ivh_softmax_axis_f32(const float* in, int n_rows, int n_cols, int64_t in_row_stride, int64_t in_col_stride, float* out,
                                    int64_t out_row_stride, int64_t out_col_stride, int mul_input, void* stream) {
  IVH_REQUIRE(in && out, "softmax_axis: null pointer");
  IVH_REQUIRE(n_rows >= 1 && n_cols >= 1, "softmax_axis: empty matrix (%d x %d)", n_rows, n_cols);
  IVH_REQUIRE(in_row_stride >= 0 && in_col_stride >= 0, "softmax_axis: negative input stride");
  // the output is written: it must be a dense matrix in one of the two orders, so that no two elements share an address
  IVH_REQUIRE((out_col_stride == 1 && out_row_stride >= n_cols) || (out_row_stride == 1 && out_col_stride >= n_rows),
              "softmax_axis: output strides (%lld, %lld) are neither row- nor column-major for %d x %d", (long long)out_row_stride,
              (long long)out_col_stride, n_rows, n_cols);
  hipLaunchKernelGGL(softmax_axis_kernel, dim3(n_rows), dim3(256), 0, (hipStream_t)stream, in, n_cols, (long)in_row_stride,
                     (long)in_col_stride, out, (long)out_row_stride, (long)out_col_stride, mul_input);
  return ivh_host::check_launch("softmax_axis");
}

// workspace: one byte per (owned video, text) pair, rounded up to whole 32-bit words, then one int32 count per owned video
extern "C" int64_t ivh_rerank_lists_workspace_bytes(int n_videos, int nt) {
  if (n_videos < 0 || nt < 0) return -1;
  return (((int64_t)n_videos * nt + 3) / 4) * 4 + (int64_t)n_videos * 4;
}

extern "C" int ivh_rerank_lists(const int32_t* idx_v2t, int nv, int kv, const int32_t* idx_t2v, int nt, int kt, int v_begin, int v_end,
                                int32_t* ptr, int32_t* cand, uint8_t* flags, void* workspace, void* stream) {
  IVH_REQUIRE(idx_v2t && idx_t2v && ptr && cand && flags && workspace, "rerank_lists: null pointer");
  IVH_REQUIRE(nv >= 1 && nt >= 1 && kv >= 1 && kt >= 1 && kv <= nt && kt <= nv, "rerank_lists: bad sizes nv %d nt %d kv %d kt %d", nv, nt, kv, kt);
  IVH_REQUIRE(0 <= v_begin && v_begin < v_end && v_end <= nv, "rerank_lists: video range [%d, %d) outside [0, %d)", v_begin, v_end, nv);
  const int n = v_end - v_begin;
  const int64_t capacity = (int64_t)n * kv + (int64_t)nt * kt;
  IVH_REQUIRE(fits_i32(capacity), "rerank_lists: %lld candidate slots do not fit the int32 row pointers", (long long)capacity);
  hipStream_t s = (hipStream_t)stream;
  const int64_t pair_bytes = (((int64_t)n * nt + 3) / 4) * 4;
  unsigned* pairs = (unsigned*)workspace;
  int* counts = (int*)((char*)workspace + pair_bytes);
  if (hipMemsetAsync(pairs, 0, (size_t)pair_bytes, s) != hipSuccess) {
    ivh_host::set_error("rerank_lists: clearing the workspace failed");
    return -1;
  }
  int64_t blocks = (capacity + 255) / 256;
  blocks = blocks > 4096 ? 4096 : blocks;
  hipLaunchKernelGGL(rerank_mark_kernel, dim3((unsigned)blocks), dim3(256), 0, s, idx_v2t, kv, idx_t2v, nt, kt, v_begin, v_end, pairs);
  hipLaunchKernelGGL(rerank_count_kernel, dim3(n), dim3(256), 0, s, (const unsigned char*)pairs, nt, counts);
  hipLaunchKernelGGL(rerank_scan_kernel, dim3(1), dim3(256), 0, s, (const int*)counts, n, ptr);
  hipLaunchKernelGGL(rerank_fill_kernel, dim3(n), dim3(256), 0, s, (const unsigned char*)pairs, nt, (const int*)ptr, (long)capacity, cand, flags);
  return ivh_host::check_launch("rerank_lists");
}

extern "C" int ivh_scatter_pair_scores(const int32_t* ptr, const int32_t* cand, const uint8_t* flags, const float* scores, int64_t capacity,
                                       int v_begin, int n_videos, int nv, int nt, float* x_v2t, int64_t v2t_row_stride,
                                       int64_t v2t_col_stride, float* x_t2v, int64_t t2v_row_stride, int64_t t2v_col_stride, void* stream) {
  IVH_REQUIRE(ptr && cand && flags && scores && x_v2t && x_t2v, "scatter_pair_scores: null pointer");
  IVH_REQUIRE(nv >= 1 && nt >= 1 && n_videos >= 1 && v_begin >= 0 && (int64_t)v_begin + n_videos <= nv,
              "scatter_pair_scores: videos [%d, %d + %d) outside [0, %d)", v_begin, v_begin, n_videos, nv);
  IVH_REQUIRE(capacity >= 0, "scatter_pair_scores: negative capacity");
  IVH_REQUIRE((v2t_col_stride == 1 && v2t_row_stride >= nt) || (v2t_row_stride == 1 && v2t_col_stride >= nv),
              "scatter_pair_scores: x_v2t strides are neither row- nor column-major for %d x %d", nv, nt);
  IVH_REQUIRE((t2v_col_stride == 1 && t2v_row_stride >= nv) || (t2v_row_stride == 1 && t2v_col_stride >= nt),
              "scatter_pair_scores: x_t2v strides are neither row- nor column-major for %d x %d", nt, nv);
  hipLaunchKernelGGL(scatter_pair_scores_kernel, dim3(n_videos), dim3(256), 0, (hipStream_t)stream, ptr, cand, flags, scores, (long)capacity,
                     v_begin, nt, x_v2t, (long)v2t_row_stride, (long)v2t_col_stride, x_t2v, (long)t2v_row_stride, (long)t2v_col_stride);
  return ivh_host::check_launch("scatter_pair_scores");
}

extern "C" int ivh_retrieval_ranks(const float* scores, int n_rows, int n_cols, int64_t row_stride, int64_t col_stride, const int32_t* gt_ptr,
                                   const int32_t* gt_idx, int32_t* rank, void* stream) {
  IVH_REQUIRE(scores && gt_ptr && gt_idx && rank, "retrieval_ranks: null pointer");
  IVH_REQUIRE(n_rows >= 1 && n_cols >= 1, "retrieval_ranks: empty matrix (%d x %d)", n_rows, n_cols);
  IVH_REQUIRE(row_stride >= 0 && col_stride >= 0, "retrieval_ranks: negative stride");
  hipLaunchKernelGGL(retrieval_ranks_kernel, dim3(n_rows), dim3(256), 0, (hipStream_t)stream, scores, n_cols, (long)row_stride,
                     (long)col_stride, gt_ptr, gt_idx, rank);
  return ivh_host::check_launch("retrieval_ranks");
}
