// Kernels of the fine-tuning step (single_modality/run_finetuning.py, engines/engine_for_finetuning.py):
//   * Mixup / CutMix of a clip batch (datasets/mixup.py:159-207), fused with the cast to bf16 (engine_for_finetuning.py:63-67).  The draw
//     (partner sample, kind, box, the two weights) is a per-sample table in DEVICE memory, so a captured step mixes with a fresh draw on
//     every replay (the same treatment as ivh_droppath_plan gives DropPath);
//   * soft-target cross entropy over the rows of the classifier's logits (timm SoftTargetCrossEntropy, run_finetuning.py:593-597; with
//     lam = 1 timm LabelSmoothingCrossEntropy), forward, gradient and the rank of the label in one launch;
//   * the dense (M, V) target of datasets/mixup.py:22-27 for callers that keep the reference's loop.
// All three are memory-bound; same idiom as bert.hip (ce_rows_kernel): 256 threads, 16-byte accesses, fp32 math, one workgroup per logits row.
// Wherever a result is pinned bit for bit to the reference's separately rounded torch ops, the products and the sum sit in a
// `#pragma clang fp contract(off)` block (mix2).  The library's -ffp-contract=fast disregards that pragma (the 2x-unrolled loop of
// mixup_target_kernel came out as v_pk_fma_f32 under it), and the header's __fmul_rn / __fadd_rn are a plain `x * y` / `x + y`; so
// csrc/build.py compiles THIS file with -ffp-contract=fast-honor-pragmas, under which mix2 is mul + mul + add by construction.
#include "common.h"
#include "../../include/internvideo_hip.h"

namespace ivh {
namespace finetune {

// rn(rn(a wa) + rn(b wb)): two rounded products, one rounded sum
__device__ __forceinline__ float mix2(float a, float wa, float b, float wb) {
#pragma clang fp contract(off)
  const float p = a * wa, q = b * wb;
  return p + q;
}

template <typename T, int VEC>
__device__ __forceinline__ void ldv(const T* p, float* o) {
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(p + 4 * q);
      o[4 * q] = a[0]; o[4 * q + 1] = a[1]; o[4 * q + 2] = a[2]; o[4 * q + 3] = a[3];
    }
  } else if constexpr (VEC == 8) {
    unpack8(*reinterpret_cast<const u32x4*>(p), o);
  } else {
    const u32x2 a = *reinterpret_cast<const u32x2*>(p);
    o[0] = __uint_as_float(a[0] << 16); o[1] = __uint_as_float(a[0] & 0xffff0000u);
    o[2] = __uint_as_float(a[1] << 16); o[3] = __uint_as_float(a[1] & 0xffff0000u);
  }
}
template <typename T, int VEC>
__device__ __forceinline__ void stv(T* p, const float* v) {
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q) *reinterpret_cast<f32x4*>(p + 4 * q) = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
  } else if constexpr (VEC == 8) {
    *reinterpret_cast<u32x4*>(p) = pack8(v);
  } else {
    *reinterpret_cast<u32x2*>(p) = pack4(v[0], v[1], v[2], v[3]);
  }
}

// One sample per blockIdx.y, N = C*T*H*W elements in chunks of VEC (N % VEC == 0: every chunk is whole and 4*VEC / 2*VEC bytes aligned).
// table[i] = {src, kind, yl, yh, xl, xh, bits(lam), bits(oml)}.  kind 1: out = rn(rn(x[i] lam) + rn(x[src] oml)); kind 2: x[src] inside the box
// [yl, yh) x [xl, xh) of every frame, x[i] outside -- a select, the other operand is not even loaded when the chunk lies on one side; any other
// kind, or a partner outside [0, B): the sample passes through.  A chunk may straddle a row end or a box edge: the decision is per element.
template <typename TI, typename TO, int VEC>
__global__ __launch_bounds__(256) void mix_clips_kernel(const TI* __restrict__ x, const int* __restrict__ table, int B, long N, int H, int W,
                                                        TO* __restrict__ out) {
  const int i = blockIdx.y;
  const int* t = table + 8 * i;
  int src = t[0], kind = t[1];
  if (src < 0 || src >= B || kind < 0 || kind > 2) kind = 0;
  const int yl = t[2], yh = t[3], xl = t[4], xh = t[5];
  const float lam = __int_as_float(t[6]), oml = __int_as_float(t[7]);
  const TI* xi = x + (long)i * N;
  const TI* xs = x + (long)(kind ? src : i) * N;
  TO* o = out + (long)i * N;
  const long nchunk = N / VEC;
  for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < nchunk; c += (long)gridDim.x * 256) {
    const long base = c * VEC;
    float a[VEC], b[VEC];
    if (kind == 0) {
      ldv<TI, VEC>(xi + base, a);
    } else if (kind == 1) {
      ldv<TI, VEC>(xi + base, a);
      ldv<TI, VEC>(xs + base, b);
#pragma unroll
      for (int e = 0; e < VEC; ++e) a[e] = mix2(a[e], lam, b[e], oml);
    } else {
      const long r = base / W;
      int px = (int)(base - r * W), py = (int)(r % H);
      bool in[VEC];
      int n_in = 0;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        in[e] = py >= yl && py < yh && px >= xl && px < xh;
        n_in += in[e];
        if (++px == W) { px = 0; if (++py == H) py = 0; }
      }
      if (n_in < VEC) ldv<TI, VEC>(xi + base, a);
      if (n_in > 0) {
        ldv<TI, VEC>(xs + base, b);
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] = in[e] ? b[e] : a[e];
      }
    }
    stv<TO, VEC>(o + base, a);
  }
}

// ---- soft-target cross entropy over rows -----------------------------------------------------------------------------------------------
__device__ __forceinline__ void online_merge(float& m, float& s, float m2, float s2) {
  const float mx = fmaxf(m, m2);
  s = (m == -INFINITY ? 0.f : s * __expf(m - mx)) + (m2 == -INFINITY ? 0.f : s2 * __expf(m2 - mx));
  m = mx;
}

// eight logits at columns base .. base + 7; columns >= V (padding, or past the row) read as -inf and are never dereferenced
template <typename TX>
__device__ __forceinline__ void ld_logits(const TX* xr, int base, int V, float* v) {
  if (base + 8 <= V) {
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

// the target of one row: factored (label_a, label_b, (lam, oml), on / off values) or a dense fp32 row
struct SoftTarget {
  const float* dense;   // row pointer or NULL
  int a, b;
  float lam, oml, on, off;
  __device__ __forceinline__ float at(int c) const {
    if (dense) return dense[c];
    return mix2(c == a ? on : off, lam, c == b ? on : off, oml);      // datasets/mixup.py:27, rounded as there
  }
};

__device__ __forceinline__ float block_sum(float v, float* sh) {        // sh[4]; every thread gets the sum
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// rows[m] = inv_m * sum_c t_c (lse - x_c);  dx[m, c] = bf16(gs * (T softmax_c - t_c)), T = sum_c t_c, zeros at c >= V;
// rank[m] = #{c : x_c > x_a} + #{c < a : x_c == x_a}.  Pass 1: online (max, sum exp) and T; pass 2 (the row comes back from L2): the loss as
// a sum of NON-NEGATIVE terms t_c ((max - x_c) + log sum) -- no lse T - sum t x cancellation at large logits --, the gradient and the rank.
template <typename TX>
__global__ __launch_bounds__(256) void soft_ce_rows_kernel(const TX* __restrict__ x, int ld, int V, const int* __restrict__ label_a,
                                                           const int* __restrict__ label_b, const float* __restrict__ mix, float on, float off,
                                                           const float* __restrict__ target, long ldt, float inv_m, float dscale,
                                                           const float* __restrict__ dscale_dev, float* __restrict__ rows,
                                                           bf16_t* __restrict__ dx, int ldd, int* __restrict__ rank) {
  __shared__ float sm[4], ss[4], sh[4];
  __shared__ int si[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const TX* xr = x + (long)row * ld;
  SoftTarget tg;
  tg.dense = target ? target + (long)row * ldt : nullptr;
  tg.a = label_a ? label_a[row] : -1;
  tg.b = label_b ? label_b[row] : tg.a;
  tg.lam = mix ? mix[2 * row] : 1.0f;
  tg.oml = mix ? mix[2 * row + 1] : 0.0f;
  tg.on = on; tg.off = off;
  const int nch = (V + 7) >> 3;
  float m = -INFINITY, s = 0.f, T = 0.f;
  for (int c = tid; c < nch; c += 256) {
    float v[8];
    ld_logits(xr, c * 8, V, v);
    float cm = v[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) cm = fmaxf(cm, v[e]);
    float cs = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      cs += __expf(v[e] - cm);                                         // exp(-inf) = 0 at the padding
      if (c * 8 + e < V) T += tg.at(c * 8 + e);
    }
    online_merge(m, s, cm, cs);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    online_merge(m, s, m2, s2);
  }
  if ((tid & 63) == 0) { sm[tid >> 6] = m; ss[tid >> 6] = s; }
  __syncthreads();
  m = sm[0]; s = ss[0];
#pragma unroll
  for (int i = 1; i < 4; ++i) online_merge(m, s, sm[i], ss[i]);
  T = block_sum(T, sh);
  const float logs = __logf(s), lse = m + logs;
  const float gs = dscale * inv_m * (dscale_dev ? dscale_dev[0] : 1.0f);
  float xa = -INFINITY;
  if (rank && tg.a >= 0 && tg.a < V) {
    if constexpr (sizeof(TX) == 4) xa = xr[tg.a];
    else xa = bf2f(xr[tg.a]);
  }
  bf16_t* dr = dx ? dx + (long)row * ldd : nullptr;
  const int nch2 = dr ? (ldd >> 3) : nch;
  float loss = 0.f;
  int above = 0;
  for (int c = tid; c < nch2; c += 256) {
    float v[8], o[8];
    const int base = c * 8;
    ld_logits(xr, base, V, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int col = base + e;
      if (col < V) {
        const float t = tg.at(col);
        loss += t * ((m - v[e]) + logs);
        o[e] = gs * (T * __expf(v[e] - lse) - t);
        above += (v[e] > xa) || (v[e] == xa && col < tg.a);
      } else o[e] = 0.f;
    }
    if (dr) *reinterpret_cast<u32x4*>(dr + base) = pack8(o);
  }
  loss = block_sum(loss, sh);
  if (tid == 0) rows[row] = inv_m * loss;
  if (rank) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o, 64);
    if ((tid & 63) == 0) si[tid >> 6] = above;
    __syncthreads();
    if (tid == 0) rank[row] = (si[0] + si[1]) + (si[2] + si[3]);
  }
}

// out[i][c] = rn(rn(v1 lam) + rn(v2 oml)), v1 = c == labels[i] ? on : off, v2 = c == labels[M-1-i] ? on : off  (datasets/mixup.py:22-27)
__global__ __launch_bounds__(256) void mixup_target_kernel(const int* __restrict__ labels, const float* __restrict__ mix, int M, int V, float on,
                                                           float off, float* __restrict__ out) {
  const long n = (long)M * V;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
    const int i = (int)(idx / V), c = (int)(idx - (long)i * V);
    out[idx] = mix2(c == labels[i] ? on : off, mix[2 * i], c == labels[M - 1 - i] ? on : off, mix[2 * i + 1]);
  }
}

}  // namespace finetune
}  // namespace ivh

using namespace ivh;
using namespace ivh::finetune;

// on / off values of the smoothed one-hot, in double and then rounded to fp32 as torch.full / scatter_ do (datasets/mixup.py:23-26)
static void smooth_values(double smoothing, int V, float* on, float* off) {
  const double o = smoothing / (double)V;
  *off = (float)o;
  *on = (float)(1.0 - smoothing + o);
}

template <typename TI, typename TO>
static void launch_mix(const void* x, const int* table, int B, long N, int H, int W, void* out, hipStream_t st) {
  if (N % 8 == 0) {
    const long nb = (N / 8 + 255) / 256;
    hipLaunchKernelGGL((mix_clips_kernel<TI, TO, 8>), dim3((unsigned)(nb < 4096 ? nb : 4096), B), dim3(256), 0, st, (const TI*)x, table, B, N, H, W, (TO*)out);
  } else {
    const long nb = (N / 4 + 255) / 256;
    hipLaunchKernelGGL((mix_clips_kernel<TI, TO, 4>), dim3((unsigned)(nb < 4096 ? nb : 4096), B), dim3(256), 0, st, (const TI*)x, table, B, N, H, W, (TO*)out);
  }
}

extern "C" int ivh_mix_clips(const void* x, int x_fp32, const int32_t* table, int B, int C, int T, int H, int W, void* out, int out_fp32,
                             void* stream) {
  IVH_REQUIRE(x && table && out && B > 0 && C > 0 && T > 0 && H > 0 && W > 0, "mix_clips: bad args");
  IVH_REQUIRE(x != out, "mix_clips: out of place only (sample i reads sample B-1-i)");
  IVH_REQUIRE(B <= 65535, "mix_clips: batch %d exceeds the grid's second dimension", B);
  const long N = (long)C * T * H * W;
  IVH_REQUIRE(N % 4 == 0, "mix_clips: C*T*H*W = %ld must be a multiple of 4", N);
  IVH_REQUIRE(((uintptr_t)x | (uintptr_t)out) % 16 == 0, "mix_clips: x and out must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (x_fp32 && out_fp32) launch_mix<float, float>(x, table, B, N, H, W, out, st);
  else if (x_fp32) launch_mix<float, bf16_t>(x, table, B, N, H, W, out, st);
  else if (out_fp32) launch_mix<bf16_t, float>(x, table, B, N, H, W, out, st);
  else launch_mix<bf16_t, bf16_t>(x, table, B, N, H, W, out, st);
  return ivh_host::check_launch("mix_clips");
}

extern "C" int ivh_soft_ce_rows(const void* logits, int logits_fp32, int ld, int M, int V, const int32_t* label_a, const int32_t* label_b,
                                const float* mix, double smoothing, const float* target, int64_t ldt, float dscale, const float* dscale_dev,
                                float* rows, float* loss, uint16_t* dlogits, int ldd, int32_t* rank, void* stream) {
  IVH_REQUIRE(logits && rows && M > 0 && V > 0 && ld >= V, "soft_ce_rows: bad args");
  IVH_REQUIRE(ld % 8 == 0 && (!dlogits || (ldd % 8 == 0 && ldd >= V)), "soft_ce_rows: leading dimensions must be multiples of 8 and >= V");
  IVH_REQUIRE((uintptr_t)logits % 16 == 0 && (uintptr_t)dlogits % 16 == 0, "soft_ce_rows: logits and dlogits must be 16-byte aligned");
  IVH_REQUIRE(target || label_a, "soft_ce_rows: give the target dense (target) or factored (label_a [, label_b, mix])");
  IVH_REQUIRE(!target || (ldt >= V && !label_b && !mix), "soft_ce_rows: a dense target has ldt >= V and comes without label_b / mix");
  IVH_REQUIRE(!rank || label_a, "soft_ce_rows: rank is the position of label_a");
  IVH_REQUIRE((const void*)dlogits != logits, "soft_ce_rows: out of place only");
  IVH_REQUIRE(smoothing >= 0.0 && smoothing <= 1.0, "soft_ce_rows: smoothing = %f outside [0, 1]", smoothing);
  float on, off;
  smooth_values(smoothing, V, &on, &off);
  const float inv_m = 1.0f / (float)M;
  hipStream_t st = (hipStream_t)stream;
  if (logits_fp32)
    hipLaunchKernelGGL(soft_ce_rows_kernel<float>, dim3(M), dim3(256), 0, st, (const float*)logits, ld, V, label_a, label_b, mix, on, off, target,
                       (long)ldt, inv_m, dscale, dscale_dev, rows, dlogits, ldd, rank);
  else
    hipLaunchKernelGGL(soft_ce_rows_kernel<bf16_t>, dim3(M), dim3(256), 0, st, (const bf16_t*)logits, ld, V, label_a, label_b, mix, on, off, target,
                       (long)ldt, inv_m, dscale, dscale_dev, rows, dlogits, ldd, rank);
  if (ivh_host::check_launch("soft_ce_rows")) return -1;
  return loss ? ivh_sum_rows(rows, M, 1.0f, loss, stream) : 0;
}

extern "C" int ivh_mixup_target(const int32_t* labels, const float* mix, int M, int V, double smoothing, float* out, void* stream) {
  IVH_REQUIRE(labels && mix && out && M > 0 && V > 0, "mixup_target: bad args");
  IVH_REQUIRE(smoothing >= 0.0 && smoothing <= 1.0, "mixup_target: smoothing = %f outside [0, 1]", smoothing);
  float on, off;
  smooth_values(smoothing, V, &on, &off);
  const long nb = ((long)M * V + 255) / 256;
  hipLaunchKernelGGL(mixup_target_kernel, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, (hipStream_t)stream, labels, mix, M, V, on, off, out);
  return ivh_host::check_launch("mixup_target");
}
