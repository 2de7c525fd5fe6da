// Linear / attentive probing heads (reference InternVideo2/single_modality/models/internvideo2_cat.py "C:", run_linear_probing.py):
//   ivh_cat_pool_fwd / _bwd         cls row + per-frame (avgN) or all-patch (avg1) means of the final residual stream (C:583-587), and
//                                   optionally the all-token mean AttentionPoolingBlock takes as its query (P:110), from ONE pass over it
//   ivh_batchnorm_cols_fwd / _bwd   `down_norm(final.permute(0, 2, 1)).reshape(B, -1)` (C:589-590): BatchNorm1d over the B * G values of a
//                                   channel, output written channel-major (c * G + g) as the head GEMM reads it
// The stream pass is bandwidth bound (1.5 GB at 1B / 16 frames / batch 64): 16-byte loads along C, fp32 accumulation over the S rows of
// a frame, one workgroup per (clip, frame, channel chunk).  No float atomics anywhere: every sum has one fixed order, so two runs agree
// bit for bit.  The batch-norm side works on a few MB that stay in L2.
#include "common.h"
#include "../../include/internvideo_hip.h"

namespace ivh {

// ---- pool ---------------------------------------------------------------------------------------------------------------------------
// VEC channels per lane (one 16-byte load): 4 for an fp32 stream, 8 for a bf16 one.  A workgroup is COLS column lanes x (256 / COLS) row
// lanes; row lane r sums rows r, r + RL, .. of its frame in that order, the row lanes are then summed through LDS in lane order.
template <bool FP32> struct PoolVec { static constexpr int V = FP32 ? 4 : 8; };

template <bool FP32>
__device__ __forceinline__ void pool_load(const void* x, size_t elem, float* v) {
  if constexpr (FP32) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(x) + elem);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else {
    const u32x4 t = *reinterpret_cast<const u32x4*>(reinterpret_cast<const bf16_t*>(x) + elem);
    unpack8(t, v);
  }
}

// grid (B * T, column chunks).  frame_mean: [B][T][C] with row pitch `fm_ld` rows per clip (out + C for avgN: rows 1 .. T of a clip's
// G = 1 + T rows; the workspace for avg1).  cls_out: [B][G][C], row 0 of every clip.
template <bool FP32, int COLS>
__global__ __launch_bounds__(256) void cat_pool_frames_kernel(const void* __restrict__ x, int T, int S, int C, float* __restrict__ frame_mean,
                                                                int fm_rows_per_clip, float* __restrict__ cls_out, int G) {
  constexpr int V = PoolVec<FP32>::V;
  constexpr int RL = 256 / COLS;
  __shared__ float part[RL][COLS][V];
  const int b = blockIdx.x / T, t = blockIdx.x % T;
  const int cl = threadIdx.x % COLS, rl = threadIdx.x / COLS;
  const int c0 = (blockIdx.y * COLS + cl) * V;
  const bool live = c0 < C;                                   // C % 8 == 0: a live lane's V channels are all inside the row
  const size_t L = 1 + (size_t)T * S;
  const size_t clip = (size_t)b * L * C;
  float acc[V];
#pragma unroll
  for (int i = 0; i < V; ++i) acc[i] = 0.f;
  if (live) {
    const size_t base = clip + ((size_t)1 + (size_t)t * S) * C + c0;
    for (int s = rl; s < S; s += RL) {
      float v[V];
      pool_load<FP32>(x, base + (size_t)s * C, v);
#pragma unroll
      for (int i = 0; i < V; ++i) acc[i] += v[i];
    }
  }
#pragma unroll
  for (int i = 0; i < V; ++i) part[rl][cl][i] = acc[i];
  __syncthreads();
  if (rl == 0 && live) {
    float sum[V];
#pragma unroll
    for (int i = 0; i < V; ++i) sum[i] = part[0][cl][i];
    for (int r = 1; r < RL; ++r) {
#pragma unroll
      for (int i = 0; i < V; ++i) sum[i] += part[r][cl][i];
    }
    float* dst = frame_mean + ((size_t)b * fm_rows_per_clip + t) * C + c0;
#pragma unroll
    for (int i = 0; i < V; ++i) dst[i] = sum[i] / (float)S;
    if (t == 0) {                                             // the cls row rides with the clip's first frame
      float v[V];
      pool_load<FP32>(x, clip + c0, v);
      float* cd = cls_out + (size_t)b * G * C + c0;
#pragma unroll
      for (int i = 0; i < V; ++i) cd[i] = v[i];
    }
  }
}

// second stage, one thread per (clip, channel): the T frame means in frame order -> the all-patch mean (avg1: out row 1) and / or the
// all-token mean (cls + S * sum_t mean_t) / L.
__global__ __launch_bounds__(256) void cat_pool_finish_kernel(const float* __restrict__ frame_mean, int fm_rows_per_clip, int B, int T, int S, int C,
                                                                const float* __restrict__ cls, int G, float* __restrict__ avg1_out,
                                                                float* __restrict__ tokmean) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * C) return;
  const int b = (int)(i / C), c = (int)(i % C);
  const float* fm = frame_mean + (size_t)b * fm_rows_per_clip * C + c;
  float acc = 0.f;
  for (int t = 0; t < T; ++t) acc += fm[(size_t)t * C];
  if (avg1_out) avg1_out[(size_t)b * G * C + C + c] = acc / (float)T;
  if (tokmean) tokmean[i] = (cls[(size_t)b * G * C + c] + acc * (float)S) / (float)(1 + (size_t)T * S);
}

// dx[b][0] (+)= dout[b][0] + dtok[b] / L;  dx[b][1 + t S + s] (+)= dmean / S + dtok[b] / L, dmean = dout[b][1 + t] (avgN) or dout[b][1] / T.
// One thread per 4 channels of one stream row.
__global__ __launch_bounds__(256) void cat_pool_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ dtok, int B, int T, int S, int C,
                                                             int mode, int accumulate, float* __restrict__ dx) {
  const int C4 = C >> 2;
  const size_t L = 1 + (size_t)T * S;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * L * C4) return;
  const int c = (int)(i % C4) * 4;
  const size_t row = i / C4;
  const int b = (int)(row / L);
  const size_t l = row % L;
  const int G = mode == 0 ? 1 + T : 2;
  f32x4 g = {0.f, 0.f, 0.f, 0.f};
  if (dout) {
    if (l == 0) {
      g = *reinterpret_cast<const f32x4*>(dout + (size_t)b * G * C + c);
    } else if (mode == 0) {
      const int t = (int)((l - 1) / S);
      g = *reinterpret_cast<const f32x4*>(dout + ((size_t)b * G + 1 + t) * C + c) / (float)S;
    } else {
      g = *reinterpret_cast<const f32x4*>(dout + ((size_t)b * G + 1) * C + c) / ((float)S * (float)T);
    }
  }
  if (dtok) g += *reinterpret_cast<const f32x4*>(dtok + (size_t)b * C + c) / (float)L;
  f32x4* d = reinterpret_cast<f32x4*>(dx + row * C + c);
  *d = accumulate ? *d + g : g;
}

// ---- batch norm over the rows of a [B][G][C] tensor, channel-major output ---------------------------------------------------------------
// A workgroup owns BN_CW channels: BN_CW column lanes x BN_RL row lanes; row lane r visits rows r, r + BN_RL, .. in order and the row lanes
// are summed through LDS in lane order.  Statistics are CENTRED (mean first, then the squared deviations from it), in fp32.
constexpr int BN_CW = 32, BN_RL = 8;

template <bool FP32>
__device__ __forceinline__ float bn_ld(const void* x, size_t i) {
  if constexpr (FP32) return reinterpret_cast<const float*>(x)[i];
  else return bf2f(reinterpret_cast<const bf16_t*>(x)[i]);
}

__device__ __forceinline__ float bn_lane_sum(float v, float (*red)[BN_CW], int rl, int cl) {
  __syncthreads();                                           // the previous call's readers are done with red
  red[rl][cl] = v;
  __syncthreads();
  float s = red[0][cl];
#pragma unroll
  for (int r = 1; r < BN_RL; ++r) s += red[r][cl];
  return s;
}

template <bool FP32>
__global__ __launch_bounds__(256) void batchnorm_cols_fwd_kernel(const void* __restrict__ x, int B, int G, int C, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, float eps, int training, float momentum,
                                                                 float* __restrict__ running_mean, float* __restrict__ running_var,
                                                                 long long* __restrict__ nbt, bf16_t* __restrict__ y, long ld_y,
                                                                 float* __restrict__ save_mean, float* __restrict__ save_rstd) {
  __shared__ float red[BN_RL][BN_CW];
  const int cl = threadIdx.x % BN_CW, rl = threadIdx.x / BN_CW;
  const int c = blockIdx.x * BN_CW + cl;
  const bool live = c < C;
  const int N = B * G;
  float mean, rstd;
  if (training) {
    float s = 0.f;
    if (live) for (int r = rl; r < N; r += BN_RL) s += bn_ld<FP32>(x, (size_t)r * C + c);
    mean = bn_lane_sum(s, red, rl, cl) / (float)N;
    float q = 0.f;
    if (live) for (int r = rl; r < N; r += BN_RL) { const float d = bn_ld<FP32>(x, (size_t)r * C + c) - mean; q += d * d; }
    const float ss = bn_lane_sum(q, red, rl, cl);
    const float var = ss / (float)N;
    rstd = 1.0f / sqrtf(var + eps);
    if (live && rl == 0) {
      if (running_mean) running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * mean;
      if (running_var) running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (ss / (float)(N - 1));
    }
    if (nbt && blockIdx.x == 0 && threadIdx.x == 0) nbt[0] += 1;
  } else {
    mean = live ? running_mean[c] : 0.f;
    rstd = live ? 1.0f / sqrtf(running_var[c] + eps) : 0.f;
  }
  if (!live) return;
  if (rl == 0) {
    if (save_mean) save_mean[c] = mean;
    if (save_rstd) save_rstd[c] = rstd;
  }
  const float ww = w ? w[c] : 1.0f, bb = bias ? bias[c] : 0.0f;
  for (int r = rl; r < N; r += BN_RL) {
    const int b = r / G, g = r % G;
    const float v = (bn_ld<FP32>(x, (size_t)r * C + c) - mean) * rstd * ww + bb;
    y[(size_t)b * ld_y + (size_t)c * G + g] = f2bf(v);
  }
}

// dx = rstd (dyw - mean(dyw) - xhat mean(dyw xhat)), dyw = dy w (training; in eval mode the statistics are constants: dx = rstd dyw);
// dw = sum dy xhat, db = sum dy.  dy is read from the flattened channel-major layout; dact (optional, bf16 [B][G][C]) multiplies dx --
// the GELU derivative of the `down` projection in front of the norm (C:457-460), which fc1's epilogue stored.
template <bool FP32, bool DXFP32>
__global__ __launch_bounds__(256) void batchnorm_cols_bwd_kernel(const void* __restrict__ x, int B, int G, int C, const float* __restrict__ w,
                                                                 const float* __restrict__ mean_, const float* __restrict__ rstd_, int training,
                                                                 const bf16_t* __restrict__ dy, long ld_dy, const bf16_t* __restrict__ dact,
                                                                 void* __restrict__ dx, float* __restrict__ dw, float* __restrict__ db) {
  __shared__ float red[BN_RL][BN_CW];
  const int cl = threadIdx.x % BN_CW, rl = threadIdx.x / BN_CW;
  const int c = blockIdx.x * BN_CW + cl;
  const bool live = c < C;
  const int N = B * G;
  const float mean = live ? mean_[c] : 0.f, rstd = live ? rstd_[c] : 0.f;
  const float ww = (live && w) ? w[c] : 1.0f;
  float s1 = 0.f, s2 = 0.f;
  if (live) {
    for (int r = rl; r < N; r += BN_RL) {
      const int b = r / G, g = r % G;
      const float d = bf2f(dy[(size_t)b * ld_dy + (size_t)c * G + g]);
      const float xh = (bn_ld<FP32>(x, (size_t)r * C + c) - mean) * rstd;
      s1 += d; s2 += d * xh;
    }
  }
  s1 = bn_lane_sum(s1, red, rl, cl);
  s2 = bn_lane_sum(s2, red, rl, cl);
  if (!live) return;
  if (rl == 0) {
    if (dw) dw[c] = s2;
    if (db) db[c] = s1;
  }
  const float m1 = training ? s1 / (float)N : 0.f, m2 = training ? s2 / (float)N : 0.f;
  for (int r = rl; r < N; r += BN_RL) {
    const int b = r / G, g = r % G;
    const float d = bf2f(dy[(size_t)b * ld_dy + (size_t)c * G + g]);
    const float xh = (bn_ld<FP32>(x, (size_t)r * C + c) - mean) * rstd;
    float v = rstd * ww * (d - m1 - xh * m2);
    if (dact) v *= bf2f(dact[(size_t)r * C + c]);
    if constexpr (DXFP32) reinterpret_cast<float*>(dx)[(size_t)r * C + c] = v;
    else reinterpret_cast<bf16_t*>(dx)[(size_t)r * C + c] = f2bf(v);
  }
}

}  // namespace ivh

using namespace ivh;

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <bool FP32>
static void launch_pool_frames(const void* x, int B, int T, int S, int C, float* fm, int fm_rows, float* cls_out, int G, hipStream_t st) {
  constexpr int V = PoolVec<FP32>::V;
  const int nvec = C / V;
  // few (clip, frame) pairs: narrow column chunks, so that C is split over more workgroups (and a frame's rows over 16 row lanes)
  if ((long)B * T * ((nvec + 63) / 64) < 512) {
    hipLaunchKernelGGL((cat_pool_frames_kernel<FP32, 16>), dim3((unsigned)(B * T), (unsigned)((nvec + 15) / 16)), dim3(256), 0, st,
                       x, T, S, C, fm, fm_rows, cls_out, G);
  } else {
    hipLaunchKernelGGL((cat_pool_frames_kernel<FP32, 64>), dim3((unsigned)(B * T), (unsigned)((nvec + 63) / 64)), dim3(256), 0, st,
                       x, T, S, C, fm, fm_rows, cls_out, G);
  }
}

extern "C" int ivh_cat_pool_fwd(const void* x, int x_fp32, int B, int T, int S, int C, int mode, float* out, float* tokmean, float* ws,
                                  void* stream) {
  IVH_REQUIRE(x && out && B > 0 && T > 0 && S > 0 && C > 0, "cat_pool_fwd: null pointer or empty shape");
  IVH_REQUIRE(C % 8 == 0, "cat_pool_fwd: C = %d must be a multiple of 8 (16-byte loads)", C);
  IVH_REQUIRE(mode == 0 || mode == 1, "cat_pool_fwd: mode %d (0 = per-frame means, 1 = one patch mean)", mode);
  IVH_REQUIRE(mode == 0 || ws, "cat_pool_fwd: mode 1 needs the [B][T][C] workspace");
  IVH_REQUIRE(aligned16(x) && aligned16(out) && aligned16(ws), "cat_pool_fwd: pointers must be 16-byte aligned");
  IVH_REQUIRE((long)B * T < 2147483647L && (long)B * C < 2147483647L * 256L, "cat_pool_fwd: grid too large");
  hipStream_t st = (hipStream_t)stream;
  const int G = mode == 0 ? 1 + T : 2;
  float* fm = mode == 0 ? out + C : ws;
  const int fm_rows = mode == 0 ? G : T;
  if (x_fp32) launch_pool_frames<true>(x, B, T, S, C, fm, fm_rows, out, G, st);
  else launch_pool_frames<false>(x, B, T, S, C, fm, fm_rows, out, G, st);
  if (mode == 1 || tokmean) {
    const size_t n = (size_t)B * C;
    hipLaunchKernelGGL(cat_pool_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, fm, fm_rows, B, T, S, C, out, G,
                       mode == 1 ? out : nullptr, tokmean);
  }
  return ivh_host::check_launch("cat_pool_fwd");
}

extern "C" int ivh_cat_pool_bwd(const float* dout, const float* dtokmean, int B, int T, int S, int C, int mode, int accumulate, float* dx,
                                  void* stream) {
  IVH_REQUIRE(dx && (dout || dtokmean) && B > 0 && T > 0 && S > 0 && C > 0, "cat_pool_bwd: null pointer or empty shape");
  IVH_REQUIRE(C % 4 == 0, "cat_pool_bwd: C = %d must be a multiple of 4 (16-byte accesses)", C);
  IVH_REQUIRE(mode == 0 || mode == 1, "cat_pool_bwd: mode %d (0 = per-frame means, 1 = one patch mean)", mode);
  IVH_REQUIRE(aligned16(dout) && aligned16(dtokmean) && aligned16(dx), "cat_pool_bwd: pointers must be 16-byte aligned");
  const size_t n = (size_t)B * (1 + (size_t)T * S) * (C / 4);
  const size_t blocks = (n + 255) / 256;
  IVH_REQUIRE(blocks < 2147483647UL, "cat_pool_bwd: grid too large");
  hipLaunchKernelGGL(cat_pool_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dout, dtokmean, B, T, S, C, mode,
                     accumulate, dx);
  return ivh_host::check_launch("cat_pool_bwd");
}

extern "C" int ivh_batchnorm_cols_fwd(const void* x, int x_fp32, int B, int G, int C, const float* w, const float* b, float eps, int training,
                                      float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked, uint16_t* y,
                                      int64_t ld_y, float* save_mean, float* save_rstd, void* stream) {
  IVH_REQUIRE(x && y && B > 0 && G > 0 && C > 0, "batchnorm_cols_fwd: null pointer or empty shape");
  IVH_REQUIRE(ld_y >= (int64_t)C * G, "batchnorm_cols_fwd: ld_y = %lld is shorter than a row of C * G = %lld", (long long)ld_y, (long long)C * G);
  IVH_REQUIRE(eps > 0.f, "batchnorm_cols_fwd: eps must be positive");
  if (training) {
    IVH_REQUIRE((long)B * G > 1, "batchnorm_cols_fwd: training needs more than one value per channel (B * G = %ld)", (long)B * G);
    IVH_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "batchnorm_cols_fwd: running_mean and running_var come together");
    IVH_REQUIRE(momentum >= 0.f && momentum <= 1.f, "batchnorm_cols_fwd: momentum %f outside [0, 1]", (double)momentum);
  } else {
    IVH_REQUIRE(running_mean && running_var, "batchnorm_cols_fwd: eval mode reads the running buffers");
  }
  IVH_REQUIRE((long)B * G < 2147483647L, "batchnorm_cols_fwd: too many rows");
  const dim3 grid((unsigned)((C + BN_CW - 1) / BN_CW));
  long long* nbt = reinterpret_cast<long long*>(training ? num_batches_tracked : nullptr);
  if (x_fp32)
    hipLaunchKernelGGL((batchnorm_cols_fwd_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, x, B, G, C, w, b, eps, training, momentum,
                       running_mean, running_var, nbt, y, (long)ld_y, save_mean, save_rstd);
  else
    hipLaunchKernelGGL((batchnorm_cols_fwd_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, x, B, G, C, w, b, eps, training, momentum,
                       running_mean, running_var, nbt, y, (long)ld_y, save_mean, save_rstd);
  return ivh_host::check_launch("batchnorm_cols_fwd");
}

extern "C" int ivh_batchnorm_cols_bwd(const void* x, int x_fp32, int B, int G, int C, const float* w, const float* mean, const float* rstd,
                                      int training, const uint16_t* dy, int64_t ld_dy, const uint16_t* dact, void* dx, int dx_fp32, float* dw,
                                      float* db, void* stream) {
  IVH_REQUIRE(x && mean && rstd && dy && dx && B > 0 && G > 0 && C > 0, "batchnorm_cols_bwd: null pointer or empty shape");
  IVH_REQUIRE(ld_dy >= (int64_t)C * G, "batchnorm_cols_bwd: ld_dy = %lld is shorter than a row of C * G = %lld", (long long)ld_dy, (long long)C * G);
  IVH_REQUIRE((long)B * G < 2147483647L, "batchnorm_cols_bwd: too many rows");
  const dim3 grid((unsigned)((C + BN_CW - 1) / BN_CW));
  hipStream_t st = (hipStream_t)stream;
#define IVH_BN_BWD(XF, DF)                                                                                                               \
  hipLaunchKernelGGL((batchnorm_cols_bwd_kernel<XF, DF>), grid, dim3(256), 0, st, x, B, G, C, w, mean, rstd, training, dy, (long)ld_dy, dact, \
                     dx, dw, db)
  if (x_fp32 && dx_fp32) IVH_BN_BWD(true, true);
  else if (x_fp32) IVH_BN_BWD(true, false);
  else if (dx_fp32) IVH_BN_BWD(false, true);
  else IVH_BN_BWD(false, false);
#undef IVH_BN_BWD
  return ivh_host::check_launch("batchnorm_cols_bwd");
}
