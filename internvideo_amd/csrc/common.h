// Shared device helpers for the gfx950 (MI355X / CDNA4) kernels of the InternVideo2 hot path.
// gfx950 only: 64-lane wavefronts, MFMA 16x16x32 bf16, LDS-DMA (global_load_lds 16 B), ds_read_b64_tr_b16.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace ivh {

typedef unsigned short bf16_t;  // storage type for bf16 in HBM / LDS
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

#define IVH_LDS __attribute__((address_space(3)))
#define IVH_GLOBAL __attribute__((address_space(1)))

constexpr int WAVE = 64;

// 16 bytes of zeros in device memory: the source for predicated-off LDS-DMA lanes (K tails, rows past
// the end, head-dim padding).  Every lane may read the same 16 bytes.
static __device__ __attribute__((aligned(16))) unsigned int g_zero_page[4] = {0u, 0u, 0u, 0u};

__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float(((unsigned)v) << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) {   // round-to-nearest-even (v_cvt_pk_bf16_f32)
  __bf16 b = (__bf16)f;
  return __builtin_bit_cast(bf16_t, b);
}
__device__ __forceinline__ u32x2 pack4(float a, float b, float c, float d) {
  f32x4 v = {a, b, c, d};
  bf16x4 r = __builtin_convertvector(v, bf16x4);
  return __builtin_bit_cast(u32x2, r);
}
__device__ __forceinline__ unsigned pack2(float a, float b) {
  f32x2 v = {a, b};
  bf16x2 r = __builtin_convertvector(v, bf16x2);
  return __builtin_bit_cast(unsigned, r);
}
__device__ __forceinline__ void unpack8(u32x4 v, float* o) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o[2 * i] = __uint_as_float(v[i] << 16);
    o[2 * i + 1] = __uint_as_float(v[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ u32x4 pack8(const float* f) {
  u32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = pack2(f[2 * i], f[2 * i + 1]);
  return r;
}

// LDS-DMA: 16 bytes per lane, LDS destination = wave-uniform base + lane*16 (hardware rule).
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const IVH_GLOBAL void*)gsrc, (IVH_LDS void*)lds_wave_base, 16, 0, 0);
}
// LDS transpose read: within each 16-lane group lane i points at 4 consecutive 16-bit elements
// (row i>>2, cols 4*(i&3)..+3 of a 4x16 block); it receives column i of that block: rows 0..3.
__device__ __forceinline__ s16x4 lds_tr16(const void* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((IVH_LDS s16x4*)p);
}
__device__ __forceinline__ f32x4 mfma16(s16x8 a, s16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float dgelu_erf(float x) {
  const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752f));
  const float pdf = 0.3989422804014327f * __expf(-0.5f * x * x);
  return cdf + x * pdf;
}
__device__ __forceinline__ float gelu_tanh(float x) {
  const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
  return 0.5f * x * (1.0f + tanhf(u));
}
__device__ __forceinline__ float dgelu_tanh(float x) {
  const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
  const float t = tanhf(u);
  const float du = 0.7978845608028654f * (1.0f + 3.0f * 0.044715f * x * x);
  return 0.5f * (1.0f + t) + 0.5f * x * (1.0f - t * t) * du;
}
// gelu_tanh(x) and gelu_tanh'(x) from ONE exp and one reciprocal (act = 4, every GEMM kernel: they agree up to accumulation order).
// With u = c (x + a x^3):  s = (1 + tanh u) / 2 = 1 / (1 + exp(-2u)),  1 - tanh^2 u = 4 s (1 - s), so
//   g = x s,   d = s + x s (1 - s) * 2c (1 + 3a x^2).
// Saturation is exact and finite while x * x is finite in fp32 (|x| < 1.8e19; the GEMM epilogues see bf16-range pre-activations of a few
// tens; beyond that d is NaN through 0 * inf, as in dgelu_tanh): exp(-2u) = +inf gives s = 0 (g = -0, d = 0), exp(-2u) = 0 gives s = 1 (g = x, d = 1); 1 - s is
// taken from the same rounded s, so s (1 - s) is never negative.  A caller that drops d pays for g alone.
__device__ __forceinline__ void gelu_tanh_pair(float x, float& g, float& d) {
  const float x2 = x * x;
  const float u2 = (-2.0f * 0.7978845608028654f) * x * fmaf(0.044715f, x2, 1.0f);       // -2u
  const float s = __builtin_amdgcn_rcpf(1.0f + __expf(u2));
  g = x * s;
  const float du2 = fmaf(2.0f * 0.7978845608028654f * 3.0f * 0.044715f, x2, 2.0f * 0.7978845608028654f);   // 2c (1 + 3a x^2)
  d = fmaf(g * (1.0f - s), du2, s);
}

// Counter-based dropout mask: keep(element) = hash(seed, 64-bit element index) >= p * 2^32.  Stateless, so forward and backward kernels
// (and a host-side check, tests/test_bert_gpu.py::dropout_keep_mask) regenerate the same mask from (seed, index) alone.
// hash = two rounds of the lowbias32 integer finaliser over the low / high index words.
__device__ __forceinline__ unsigned ivh_hash32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}
// `epoch` (device pointer or NULL, ivh_set_dropout_epoch): a step counter that lives in HBM.  A launch argument is frozen into a captured
// HIP graph, so a replayed step would draw the SAME masks every time; the effective seed is seed + *epoch * 0x9E3779B1 and the training
// engine advances *epoch with a kernel inside the captured step (forward and backward of one step read the same value).
struct DropCfg { unsigned thresh; float inv_keep; unsigned seed; const unsigned* epoch; };   // thresh = p * 2^32 (0 = no dropout), inv_keep = 1 / (1 - p)
__device__ __forceinline__ float drop_scale(const DropCfg& d, unsigned long long idx) {
  const unsigned seed = d.epoch ? d.seed + d.epoch[0] * 0x9E3779B1U : d.seed;
  const unsigned h = ivh_hash32(ivh_hash32((unsigned)idx ^ seed) ^ (unsigned)(idx >> 32) ^ 0x9e3779b9U);
  return h >= d.thresh ? d.inv_keep : 0.0f;
}

// XCD-aware, bijective remap of a linear workgroup id (block b runs on XCD b % 8): every XCD gets a
// contiguous range of the remapped ids so that neighbouring tiles share an L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = bid & 7, local = bid >> 3;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + local;
}

}  // namespace ivh

// ---- host side error plumbing (C-ABI functions return 0 on success, <0 on error) ------------------
namespace ivh_host {
void set_error(const char* fmt, ...);
int check_launch(const char* what);
const unsigned* dropout_epoch();          // device pointer registered with ivh_set_dropout_epoch, or NULL

// ---- launch geometry of the row kernels (norms.hip, bert.hip): a row of D elements is D / 8 chunks of 16 bytes -----------------------
inline int nch_for(int D) { return (D / 8 + 63) / 64; }                   // chunks per lane when ONE wave holds the row
inline int row_grid(int M, int cap) { int g = (M + 3) / 4; return g < cap ? (g < 1 ? 1 : g) : cap; }   // four rows per workgroup and trip
template <int V> using int_c = std::integral_constant<int, V>;
// The width map, the only one: nch = nch_for(D) -> the <NCH, WPR> a row kernel is instantiated with.  Up to 4 chunks a wave per row
// (<nch, 1>), 5 .. 8 the four waves of a workgroup share the row (<2, 4>).  fn(N, W) receives them as int_c values (N() and W() are constant
// expressions); false, with fn not called, for nch outside 1 .. max_nch: the caller owns the message.
template <typename F>
inline bool for_row_width(int nch, int max_nch, F&& fn) {
  switch (nch <= max_nch ? nch : 0) {
    case 1: fn(int_c<1>{}, int_c<1>{}); return true;
    case 2: fn(int_c<2>{}, int_c<1>{}); return true;
    case 3: fn(int_c<3>{}, int_c<1>{}); return true;
    case 4: fn(int_c<4>{}, int_c<1>{}); return true;
    case 5: case 6: case 7: case 8: fn(int_c<2>{}, int_c<4>{}); return true;
    default: return false;
  }
}
// one launch through the width map: fn(N, W) launches, `what` names it to check_launch; `too_wide` is the caller's message for a row the
// map has no kernel for (one %d: the width in elements)
template <typename F>
inline int launch_row_width(const char* what, int nch, int max_nch, const char* too_wide, F&& fn) {
  if (for_row_width(nch, max_nch, fn)) return check_launch(what);
  set_error(too_wide, nch * 512);
  return -1;
}

// ---- attention launches (flash_attn.hip: entry points, routes, the 16x16x32 kernels; flash_attn32.hip: switches, the 32x32x16 kernels) ----
// Everything the six ivh_flash_attn_* entry points receive.  Pointers a direction does not take are NULL, strides it does not take 0.
struct AttnArgs {
  const uint16_t *q, *k, *v;
  uint16_t* out;                                   // written by the forward, read by the backward
  const uint16_t* dout;
  float *lse, *delta;
  uint16_t *dq, *dk, *dv;
  int64_t qsb, qsl, qsh, sb, sl, sh, ob, ol, oh, dqb, dql, dqh, dsb, dsl, dsh;   // q; k and v; out and dout; dq; dk and dv
  int B, H, Lq, Lk, hd;
  float scale;
  const int32_t *kv_len, *nb_dev;
  bool dropout;                                    // a *_dropout entry point (p_drop = 0 is still that entry point)
  float p_drop;
  uint32_t seed;
  const float *qkn_rq, *qkn_rk, *qkn_wqk;          // ivh_probe_attn32_fwd_qkn only
  void* stream;
};
// the arguments every attention entry point shares; the rest of AttnArgs stays NULL / 0
inline AttnArgs attn_args(const uint16_t* q, int64_t qsb, int64_t qsl, int64_t qsh, const uint16_t* k, const uint16_t* v, int64_t sb, int64_t sl, int64_t sh,
                          int64_t ob, int64_t ol, int64_t oh, int B, int H, int Lq, int Lk, int hd, float scale, const int32_t* kv_len, void* stream) {
  AttnArgs a{};
  a.q = q; a.k = k; a.v = v;
  a.qsb = qsb; a.qsl = qsl; a.qsh = qsh; a.sb = sb; a.sl = sl; a.sh = sh; a.ob = ob; a.ol = ol; a.oh = oh;
  a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk; a.hd = hd; a.scale = scale; a.kv_len = kv_len; a.stream = stream;
  return a;
}
enum AttnKind { ATTN_FWD = 0, ATTN_DQ = 1, ATTN_DKDV = 2, ATTN_FWD2 = 3 };   // FWD2: the forward as two wave groups (attn32pp_*)
// template arguments / kernel flavours; STAMP on ATTN_FWD is no template argument: the kernel receives the stamp buffer
enum AttnFlag { ATTN_DROP = 1, ATTN_DEFER = 2, ATTN_NP = 4, ATTN_NP2 = 8, ATTN_PRIO = 16, ATTN_GSEL = 32, ATTN_STAMP = 64, ATTN_QKN = 128 };
struct AttnLaunch { int family, kind, hdp, flags; unsigned grid, block, lds; const char* what; };   // family 16 | 32; `what` names it to check_launch
struct AttnRoute { int n; AttnLaunch launch[2]; };                                                   // backward: dQ, then dK/dV
inline int attn_hdp(int hd) { return hd <= 64 ? 64 : hd <= 96 ? 96 : 128; }
// the process-wide measurement switches of the 32x32 kernels, environment defaults (IVH_ATTN_PP, IVH_ATTN_NOPK, IVH_ATTN_DEFER) resolved
struct Attn32Switches { int pingpong; bool unpacked, defer, stamps; long stamp_rows; };
Attn32Switches attn32_switches();
int attn32_supported(const AttnArgs& a);
int attn32_dkdv_lds_bytes(int Lq, int hd);
int attn32_launch(const AttnArgs& a, const AttnLaunch& l);
}  // namespace ivh_host

// ---- internals of the 256x256 GEMM (gemm256.hip) that gemm.hip / gemm_fp8.hip route through; not part of the C ABI headers --------
#include "../../include/internvideo_hip.h"
extern "C" {
int ivh_gemm256_supported(const ivh_gemm_desc* d);                            // the epilogue / layout combinations the bf16 kernel is built for
int ivh_gemm256_fits(const ivh_gemm_desc* d);                                 // every (batched) operand / output below 2 GiB - 16 MiB
int ivh_gemm256_launch(const ivh_gemm_desc* d, void* stream);
int ivh_gemm256_fp8_launch(const ivh_gemm_desc* d, const float* scale_a, const float* scale_b, int scale_b_vec, int force, void* stream);
int ivh_gemm256_grouped_launch(const ivh_gemm_desc* d, int n, void* stream);
int64_t ivh_gemm256_split_ws_bytes(const ivh_gemm_desc* d, int fp8);          // workspace with which the tail round is split along K (0 = no split)
double ivh_gemm256_split_tail_frac(const ivh_gemm_desc* d, int fp8);          // K steps of the split tail round relative to a whole round
}

#define IVH_REQUIRE(cond, ...)            \
  do {                                    \
    if (!(cond)) {                        \
      ivh_host::set_error(__VA_ARGS__);   \
      return -1;                          \
    }                                     \
  } while (0)
