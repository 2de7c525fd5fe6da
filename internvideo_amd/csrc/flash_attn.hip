// Non-causal softmax attention for equal-length video-token sequences, gfx950.
//
// Forward : O = softmax(Q K^T * scale) V          (flash style: online softmax, S never leaves registers)
// Backward: two recompute kernels, no atomics, deterministic:
//            dq  : one workgroup per 64-query tile, loops over key tiles  -> dQ (and delta = <dO, O> per query, from its prologue)
//            dkdv: one workgroup per 64-key tile, loops over query tiles  -> dK, dV
//
// Head dims 64 / 88 (InternVideo2-1B: 1408 / 16) / 128 are handled by padding the contraction to HDP = 64 / 96 /
// 128 with zero chunks supplied at staging time (the padded columns never touch HBM).
//
// MFMA plan (16x16x32 bf16, 4 waves x 16 rows): the score tile is computed TRANSPOSED, S^T = K Q^T, so that a
// lane owns one query column (softmax statistics are per lane, reduced over the 4 lane groups with two
// shuffles) and the 4 consecutive keys a lane holds per 16-key tile are exactly the k-slots the next MFMA
// (O^T += V^T P^T) wants for its B operand: P goes from accumulator to operand registers with a bf16 pack
// and no cross-lane traffic.  V^T / K^T / Q^T / dO^T A-operands are produced from the ROW-MAJOR tiles in LDS
// with ds_read_b64_tr_b16, so no transposed copy of any activation exists in HBM.
#include <type_traits>
#include "common.h"
#include "../../include/internvideo_hip.h"

namespace ivh {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

constexpr int ATTN_FWD_QW = 1;

// v_exp_f32 as it is (2^x, denormal results flushed): libm's exp2f() wraps it in a range test, two selects, an add and an ldexp --
// six VALU issues per probability instead of one, in the innermost loop of all three attention kernels
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }


template <int HDP> struct AttnCfg {
  static constexpr int RS = HDP * 2 + 32;          // LDS row stride in bytes.  +32: both the b128 row reads (4 x 16-lane groups) and the
                                                   // b64 transposing reads (2 x 32-lane groups) are conflict-free for HDP 64 / 96 / 128 under the
                                                   // gfx950 bank map ((addr / 4) mod 64); +16 was 2-way on every read (tools/lds_bank_sim.py)
  static constexpr int CPR = HDP / 8;              // 16-byte chunks per row
  static constexpr int CPT = (64 * CPR) / 256;     // chunks per thread per 64-row tile
  static constexpr int KS = HDP / 32;              // k-steps over the head dim
  static constexpr int DT = HDP / 16;              // 16-wide output tiles over the head dim
  static constexpr int TILE = 64 * RS;
};

// global -> registers for one 64 x HDP tile (rows row0.. of a (b,h) slice); zero for rows >= nrows / cols >= hd
template <int HDP>
__device__ __forceinline__ void tile_load(const bf16_t* __restrict__ base, long sl, int row0, int nrows, int hd,
                                          u32x4* regs, int tid) {
  using C = AttnCfg<HDP>;
#pragma unroll
  for (int i = 0; i < C::CPT; ++i) {
    const int id = tid + 256 * i;
    const int r = id / C::CPR, cc = id % C::CPR;
    const int row = row0 + r;
    if (row < nrows && cc * 8 < hd) regs[i] = *reinterpret_cast<const u32x4*>(base + (long)row * sl + cc * 8);
    else regs[i] = u32x4{0u, 0u, 0u, 0u};
  }
}
template <int HDP>
__device__ __forceinline__ void tile_store(char* lds_tile, const u32x4* regs, int tid) {
  using C = AttnCfg<HDP>;
#pragma unroll
  for (int i = 0; i < C::CPT; ++i) {
    const int id = tid + 256 * i;
    const int r = id / C::CPR, cc = id % C::CPR;
    *reinterpret_cast<u32x4*>(lds_tile + r * C::RS + cc * 16) = regs[i];
  }
}
// operand fragment straight from HBM: row (one per lane & 15), 8 contiguous head-dim elements at 32*ks + 8*g
template <int HDP>
__device__ __forceinline__ void row_frags(const bf16_t* __restrict__ base, long sl, int row, int nrows, int hd,
                                          s16x8* f, int lane) {
  using C = AttnCfg<HDP>;
  const int g = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < C::KS; ++ks) {
    const int d = 32 * ks + 8 * g;
    if (row < nrows && d < hd) f[ks] = *reinterpret_cast<const s16x8*>(base + (long)row * sl + d);
    else f[ks] = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
  }
}
// A operand [16 rows x 32 head-dim] of rows rbase.. from a row-major LDS tile
template <int HDP>
__device__ __forceinline__ s16x8 frag_rows(const char* tile, int rbase, int ks, int lane) {
  using C = AttnCfg<HDP>;
  return *reinterpret_cast<const s16x8*>(tile + (rbase + (lane & 15)) * C::RS + (32 * ks + 8 * (lane >> 4)) * 2);
}
// A operand [16 head-dim x 32 rows] = transposed read: head-dim cols 16*dt.., k-slots 8g+e <-> rows
// 32c + 4g + e (e < 4), 32c + 16 + 4g + e - 4 (e >= 4): the slot order of the packed S^T / S accumulators.
template <int HDP>
__device__ __forceinline__ s16x8 frag_cols_tr(const char* tile, int dt, int c, int lane) {
  using C = AttnCfg<HDP>;
  const int i = lane & 15, g = lane >> 4;
  const char* p = tile + (32 * c + 4 * g + (i >> 2)) * C::RS + (16 * dt + 4 * (i & 3)) * 2;
  const s16x4 t0 = lds_tr16(p);
  const s16x4 t1 = lds_tr16(p + 16 * C::RS);
  s16x8 r;
  r[0] = t0[0]; r[1] = t0[1]; r[2] = t0[2]; r[3] = t0[3];
  r[4] = t1[0]; r[5] = t1[1]; r[6] = t1[2]; r[7] = t1[3];
  return r;
}
__device__ __forceinline__ s16x8 pack_frag(const f32x4& lo, const f32x4& hi) {
  const u32x2 a = pack4(lo[0], lo[1], lo[2], lo[3]);
  const u32x2 b = pack4(hi[0], hi[1], hi[2], hi[3]);
  const u32x4 v = {a[0], a[1], b[0], b[1]};
  return __builtin_bit_cast(s16x8, v);
}

// =========================================================================================================
// Forward.  64 * QW queries per workgroup: each of the 4 waves owns QW 16-query column blocks, so every K fragment (ds_read_b128)
// and every transposed V fragment (2 x ds_read_b64_tr_b16) read from LDS feeds QW MFMAs.  Measured on the 1B shape (L = 417,
// hd 88): QW = 2 halves the LDS reads per MFMA but needs 208 VGPRs (2 waves / SIMD) and 4 x 128-query tiles for 417 queries
// (18 % padding instead of 7 %): 113 us against 106 us for QW = 1, so QW = 1 it is.
// DROP: dropout on the attention probabilities (BERT's attention_probs_dropout_prob, xbert.py:361,469): the probabilities that multiply V
// are masked / rescaled element by element (mask = hash(seed, ((b H + h) Lq + query) Lk_max + key), common.h), the softmax normaliser and
// the saved lse stay those of the undropped row -- O = (softmax(S) o M) V.  The backward kernels regenerate the same mask.
template <int HDP, bool DROP = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(HDP <= 96 ? 4 : 3))) void attn_fwd_kernel(const bf16_t* __restrict__ q, long qsb, long qsl, long qsh,
                                                       const bf16_t* __restrict__ k,
                                                       const bf16_t* __restrict__ v, long sb, long sl, long sh,
                                                       bf16_t* __restrict__ out, long ob, long ol, long oh,
                                                       float* __restrict__ lse, int H, int Lq, int Lk_max, int hd, float scale,
                                                       const int32_t* __restrict__ kv_len, DropCfg drop = DropCfg{0u, 1.0f, 0u}) {
  using C = AttnCfg<HDP>;
  constexpr int QW = ATTN_FWD_QW;                        // 16-query blocks per wave
  __shared__ __attribute__((aligned(16))) char lds[2 * C::TILE];
  char* Kt = lds;
  char* Vt = lds + C::TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  // 1-D grid, XCD-contiguous remap, query tile fastest: the tiles of one (b, h) run on ONE XCD and share its L2 copy of K / V.
  const int ntq = (Lq + 64 * QW - 1) / (64 * QW);
  const int wid = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = wid / ntq;
  const int b = bh / H, h = bh - b * H, q0 = (wid - bh * ntq) * 64 * QW;
  const int Lk = kv_len ? max(1, min(kv_len[b], Lk_max)) : Lk_max;      // right-padded batches: clip b has kv_len[b] valid keys
  const bf16_t* qb = q + (long)b * qsb + (long)h * qsh;
  const bf16_t* kb = k + (long)b * sb + (long)h * sh;
  const bf16_t* vb = v + (long)b * sb + (long)h * sh;

  s16x8 qf[QW][C::KS];
  f32x4 o[QW][C::DT];
  float m[QW], l[QW];
  int qrow[QW];
#pragma unroll
  for (int w = 0; w < QW; ++w) {
    qrow[w] = q0 + (wave * QW + w) * 16 + (lane & 15);
    row_frags<HDP>(qb, qsl, qrow[w], Lq, hd, qf[w], lane);
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) o[w][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    m[w] = -INFINITY; l[w] = 0.f;
  }
  const float c2 = scale * LOG2E;

  u32x4 kr[C::CPT], vr[C::CPT];
  tile_load<HDP>(kb, sl, 0, Lk, hd, kr, tid);
  tile_load<HDP>(vb, sl, 0, Lk, hd, vr, tid);
  const int nt = (Lk + 63) / 64;
  // one key tile; RAGGED (compile time) only for the last one: the bounds tests / selects of the masking are ~20 % of the loop's VALU
  auto tile = [&](const int t, auto ragged_tag) __attribute__((always_inline)) {
    constexpr bool RAGGED = decltype(ragged_tag)::value;
    __syncthreads();                       // every wave is done reading the previous tile
    tile_store<HDP>(Kt, kr, tid);
    tile_store<HDP>(Vt, vr, tid);
    __syncthreads();
    if (!RAGGED) {                         // next tile's HBM reads fly under this tile's MFMAs (the ragged tile is the last)
      tile_load<HDP>(kb, sl, (t + 1) * 64, Lk, hd, kr, tid);
      tile_load<HDP>(vb, sl, (t + 1) * 64, Lk, hd, vr, tid);
    }
    // S^T tiles: rows = keys 16j + 4g + r, col = this lane's query (one per 16-query block)
    f32x4 s[QW][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int w = 0; w < QW; ++w) s[w][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) {
        const s16x8 kfrag = frag_rows<HDP>(Kt, 16 * j, ks, lane);
#pragma unroll
        for (int w = 0; w < QW; ++w) s[w][j] = mfma16(kfrag, qf[w][ks], s[w][j]);
      }
    }
    s16x8 pf[QW][2];
#pragma unroll
    for (int w = 0; w < QW; ++w) {
      float mt = -INFINITY;                               // max of the RAW scores: the scale enters once, in the exp2 fma
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if constexpr (RAGGED) {
            const int key = t * 64 + 16 * j + 4 * g + r;
            if (key >= Lk) s[w][j][r] = -INFINITY;
          }
          mt = fmaxf(mt, s[w][j][r]);
        }
      mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      const float mn = fmaxf(m[w], mt * c2);              // c2 > 0
      const float alpha = fast_exp2(m[w] - mn);
      m[w] = mn;
      float ps = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) { s[w][j][r] = fast_exp2(fmaf(s[w][j][r], c2, -mn)); ps += s[w][j][r]; }
      l[w] = l[w] * alpha + ps;
      if constexpr (DROP) {
        const unsigned long long rowbase = ((unsigned long long)bh * Lq + qrow[w]) * (unsigned long long)Lk_max;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) s[w][j][r] *= drop_scale(drop, rowbase + (unsigned)(t * 64 + 16 * j + 4 * g + r));
      }
#pragma unroll
      for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[w][dt][r] *= alpha;
      pf[w][0] = pack_frag(s[w][0], s[w][1]);
      pf[w][1] = pack_frag(s[w][2], s[w][3]);
    }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int dt = 0; dt < C::DT; ++dt) {
        const s16x8 vfrag = frag_cols_tr<HDP>(Vt, dt, c, lane);
#pragma unroll
        for (int w = 0; w < QW; ++w) o[w][dt] = mfma16(vfrag, pf[w][c], o[w][dt]);
      }
  };
  for (int t = 0; t + 1 < nt; ++t) tile(t, std::false_type{});
  tile(nt - 1, std::true_type{});
#pragma unroll
  for (int w = 0; w < QW; ++w) {
    float lw = l[w];
    lw += __shfl_xor(lw, 16, 64);
    lw += __shfl_xor(lw, 32, 64);
    const float inv = 1.0f / lw;
    if (qrow[w] < Lq) {
      if (g == 0 && lse) lse[((long)b * H + h) * Lq + qrow[w]] = m[w] * LN2 + logf(lw);
      bf16_t* op = out + (long)b * ob + (long)qrow[w] * ol + (long)h * oh;
#pragma unroll
      for (int dt = 0; dt < C::DT; ++dt) {
        const int d = 16 * dt + 4 * g;
        if (d < hd) *reinterpret_cast<u32x2*>(op + d) = pack4(o[w][dt][0] * inv, o[w][dt][1] * inv, o[w][dt][2] * inv, o[w][dt][3] * inv);
      }
    }
  }
}

// =========================================================================================================
// dK, dV for one 64-key tile; each wave owns 16 keys (one per lane & 15) and loops over all query tiles.
template <int HDP, bool DROP = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_bwd_dkdv_kernel(
    const bf16_t* __restrict__ q, long qsb, long qsl, long qsh,
    const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, long sb, long sl, long sh,
    const bf16_t* __restrict__ dout, long ob, long ol, long oh, const float* __restrict__ lse, const float* __restrict__ delta,
    bf16_t* __restrict__ dk, bf16_t* __restrict__ dv, long dsb, long dsl, long dsh,
    int H, int Lq, int Lk, int hd, float scale, const int32_t* __restrict__ kv_len, DropCfg drop = DropCfg{0u, 1.0f, 0u},
    const int32_t* __restrict__ nb_dev = nullptr) {
  using C = AttnCfg<HDP>;
  __shared__ __attribute__((aligned(16))) char lds[2 * C::TILE + 512];
  char* Qt = lds;
  char* Dt = lds + C::TILE;
  float* lse_s = reinterpret_cast<float*>(lds + 2 * C::TILE);
  float* del_s = lse_s + 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  const int ntk = (Lk + 63) >> 6;                        // same XCD-aware 1-D grid as the forward: key tile fastest
  int nwg = gridDim.x;                                   // device-side clip count (ivh_flash_attn_bwd_dyn: head dims above 96 take this dK / dV
  if (nb_dev) {                                          // kernel): the remap runs over the REAL grid, see attn32_fwd_kernel
    nwg = min(nwg, ntk * H * max(0, *nb_dev));
    if ((int)blockIdx.x >= nwg) return;
  }
  const int wid = xcd_remap(blockIdx.x, nwg);
  const int bh = wid / ntk;
  const int b = bh / H, h = bh - b * H, k0 = (wid - bh * ntk) * 64;
  const bf16_t* qb = q + (long)b * qsb + (long)h * qsh;
  const bf16_t* kb = k + (long)b * sb + (long)h * sh;
  const bf16_t* vb = v + (long)b * sb + (long)h * sh;
  const bf16_t* dob = dout + (long)b * ob + (long)h * oh;
  const float* lseb = lse + ((long)b * H + h) * Lq;
  const float* delb = delta + ((long)b * H + h) * Lq;
  const int key = k0 + wave * 16 + (lane & 15);
  const int Lk_b = kv_len ? max(1, min(kv_len[b], Lk)) : Lk;            // keys >= Lk_b are padding: their dK / dV rows are written as zeros

  s16x8 kf[C::KS], vf[C::KS];
  row_frags<HDP>(kb, sl, key, Lk_b, hd, kf, lane);
  row_frags<HDP>(vb, sl, key, Lk_b, hd, vf, lane);
  f32x4 dkt[C::DT], dvt[C::DT];
#pragma unroll
  for (int dt = 0; dt < C::DT; ++dt) { dkt[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dvt[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  const float c2 = scale * LOG2E;

  u32x4 qr[C::CPT], dr[C::CPT];
  tile_load<HDP>(qb, qsl, 0, Lq, hd, qr, tid);
  tile_load<HDP>(dob, ol, 0, Lq, hd, dr, tid);
  const int nt = (Lq + 63) / 64;
  for (int t = 0; t < nt; ++t) {
    __syncthreads();
    tile_store<HDP>(Qt, qr, tid);
    tile_store<HDP>(Dt, dr, tid);
    if (tid < 64) {
      const int qi = t * 64 + tid;
      lse_s[tid] = qi < Lq ? lseb[qi] * LOG2E : INFINITY;    // +inf -> P = 0 for padded queries
      del_s[tid] = qi < Lq ? delb[qi] : 0.f;
    }
    __syncthreads();
    if (t + 1 < nt) {
      tile_load<HDP>(qb, qsl, (t + 1) * 64, Lq, hd, qr, tid);
      tile_load<HDP>(dob, ol, (t + 1) * 64, Lq, hd, dr, tid);
    }
    // S and dP tiles: rows = queries 16qi + 4g + r, col = this lane's key
    f32x4 p[4], ds[4];
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) {
        s = mfma16(frag_rows<HDP>(Qt, 16 * qi, ks, lane), kf[ks], s);
        dp = mfma16(frag_rows<HDP>(Dt, 16 * qi, ks, lane), vf[ks], dp);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qq = 16 * qi + 4 * g + r;
        const float pv = fast_exp2(s[r] * c2 - lse_s[qq]);
        if constexpr (DROP) {                                  // dV sees the dropped probabilities, dS the dropped dP (delta already does)
          const float mk = drop_scale(drop, ((unsigned long long)bh * Lq + (unsigned)(t * 64 + qq)) * (unsigned long long)Lk + (unsigned)key);
          p[qi][r] = pv * mk;
          ds[qi][r] = pv * (dp[r] * mk - del_s[qq]);
        } else {
          p[qi][r] = pv;
          ds[qi][r] = pv * (dp[r] - del_s[qq]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const s16x8 pf = pack_frag(p[2 * c], p[2 * c + 1]);
      const s16x8 dsf = pack_frag(ds[2 * c], ds[2 * c + 1]);
#pragma unroll
      for (int dt = 0; dt < C::DT; ++dt) {
        dvt[dt] = mfma16(frag_cols_tr<HDP>(Dt, dt, c, lane), pf, dvt[dt]);
        dkt[dt] = mfma16(frag_cols_tr<HDP>(Qt, dt, c, lane), dsf, dkt[dt]);
      }
    }
  }
  if (key < Lk) {
    bf16_t* dkp = dk + (long)b * dsb + (long)key * dsl + (long)h * dsh;
    bf16_t* dvp = dv + (long)b * dsb + (long)key * dsl + (long)h * dsh;
    const float live = key < Lk_b ? 1.0f : 0.0f;
    const float ks_ = scale * live;
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) {
      const int d = 16 * dt + 4 * g;
      if (d < hd) {
        *reinterpret_cast<u32x2*>(dkp + d) = pack4(dkt[dt][0] * ks_, dkt[dt][1] * ks_, dkt[dt][2] * ks_, dkt[dt][3] * ks_);
        *reinterpret_cast<u32x2*>(dvp + d) = pack4(dvt[dt][0] * live, dvt[dt][1] * live, dvt[dt][2] * live, dvt[dt][3] * live);
      }
    }
  }
}

// =========================================================================================================
// dQ for one 64-query tile; each wave owns 16 queries (one per lane & 15) and loops over all key tiles.
template <int HDP, bool DROP = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(HDP <= 64 ? 4 : (HDP <= 96 ? 3 : 2)))) void attn_bwd_dq_kernel(
    const bf16_t* __restrict__ q, long qsb, long qsl, long qsh,
    const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, long sb, long sl, long sh,
    const bf16_t* __restrict__ out, const bf16_t* __restrict__ dout, long ob, long ol, long oh, const float* __restrict__ lse,
    float* __restrict__ delta, bf16_t* __restrict__ dq, long dqb, long dql, long dqh, int H, int Lq, int Lk_max, int hd, float scale,
    const int32_t* __restrict__ kv_len, DropCfg drop = DropCfg{0u, 1.0f, 0u}) {
  using C = AttnCfg<HDP>;
  __shared__ __attribute__((aligned(16))) char lds[2 * C::TILE];
  char* Kt = lds;
  char* Vt = lds + C::TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  const int ntq = (Lq + 63) >> 6;
  const int wid = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = wid / ntq;
  const int b = bh / H, h = bh - b * H, q0 = (wid - bh * ntq) * 64;
  const int Lk = kv_len ? max(1, min(kv_len[b], Lk_max)) : Lk_max;
  const bf16_t* qb = q + (long)b * qsb + (long)h * qsh;
  const bf16_t* kb = k + (long)b * sb + (long)h * sh;
  const bf16_t* vb = v + (long)b * sb + (long)h * sh;
  const bf16_t* dob = dout + (long)b * ob + (long)h * oh;
  const int qrow = q0 + wave * 16 + (lane & 15);

  s16x8 qf[C::KS], dof[C::KS];
  row_frags<HDP>(qb, qsl, qrow, Lq, hd, qf, lane);
  row_frags<HDP>(dob, ol, qrow, Lq, hd, dof, lane);
  const float lse2 = qrow < Lq ? lse[((long)b * H + h) * Lq + qrow] * LOG2E : INFINITY;
  // delta[q] = <dO[q], O[q]>: the lane holds 8 * KS elements of its query row (the other three 16-lane groups hold the rest), so the
  // row dot product is a register loop and two shuffles -- no separate pass over O and dO.  Written out for the dK/dV kernel.
  float del = 0.f;
  {
    s16x8 of[C::KS];
    row_frags<HDP>(out + (long)b * ob + (long)h * oh, ol, qrow, Lq, hd, of, lane);
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) {
      float a[8], g8[8];
      unpack8(__builtin_bit_cast(u32x4, of[ks]), a);
      unpack8(__builtin_bit_cast(u32x4, dof[ks]), g8);
#pragma unroll
      for (int e = 0; e < 8; ++e) del += a[e] * g8[e];
    }
    del += __shfl_xor(del, 16, 64);
    del += __shfl_xor(del, 32, 64);
    if (g == 0 && qrow < Lq) delta[((long)b * H + h) * Lq + qrow] = del;
  }
  f32x4 dqt[C::DT];
#pragma unroll
  for (int dt = 0; dt < C::DT; ++dt) dqt[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float c2 = scale * LOG2E;

  u32x4 kr[C::CPT], vr[C::CPT];
  tile_load<HDP>(kb, sl, 0, Lk, hd, kr, tid);
  tile_load<HDP>(vb, sl, 0, Lk, hd, vr, tid);
  const int nt = (Lk + 63) / 64;
  auto tile = [&](const int t, auto ragged_tag) __attribute__((always_inline)) {
    constexpr bool RAGGED = decltype(ragged_tag)::value;
    __syncthreads();
    tile_store<HDP>(Kt, kr, tid);
    tile_store<HDP>(Vt, vr, tid);
    __syncthreads();
    if (!RAGGED) {
      tile_load<HDP>(kb, sl, (t + 1) * 64, Lk, hd, kr, tid);
      tile_load<HDP>(vb, sl, (t + 1) * 64, Lk, hd, vr, tid);
    }
    f32x4 ds[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) {
        s = mfma16(frag_rows<HDP>(Kt, 16 * j, ks, lane), qf[ks], s);
        dp = mfma16(frag_rows<HDP>(Vt, 16 * j, ks, lane), dof[ks], dp);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float pv = fast_exp2(s[r] * c2 - lse2);
        if constexpr (RAGGED) {
          const int key = t * 64 + 16 * j + 4 * g + r;
          if (key >= Lk) pv = 0.f;
        }
        float dpr = dp[r];
        if constexpr (DROP)
          dpr *= drop_scale(drop, ((unsigned long long)bh * Lq + (unsigned)qrow) * (unsigned long long)Lk_max + (unsigned)(t * 64 + 16 * j + 4 * g + r));
        ds[j][r] = pv * (dpr - del);
      }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const s16x8 dsf = pack_frag(ds[2 * c], ds[2 * c + 1]);
#pragma unroll
      for (int dt = 0; dt < C::DT; ++dt) dqt[dt] = mfma16(frag_cols_tr<HDP>(Kt, dt, c, lane), dsf, dqt[dt]);
    }
  };
  for (int t = 0; t + 1 < nt; ++t) tile(t, std::false_type{});
  tile(nt - 1, std::true_type{});
  if (qrow < Lq) {
    bf16_t* dqp = dq + (long)b * dqb + (long)qrow * dql + (long)h * dqh;
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) {
      const int d = 16 * dt + 4 * g;
      if (d < hd) *reinterpret_cast<u32x2*>(dqp + d) = pack4(dqt[dt][0] * scale, dqt[dt][1] * scale, dqt[dt][2] * scale, dqt[dt][3] * scale);
    }
  }
}

}  // namespace ivh

using namespace ivh;
using namespace ivh_host;

// 0 = automatic (the 32x32 kernels whenever they support the problem), 1 = the 16x16x32 kernels of this file, 2 = 32x32 or error
static int g_attn_impl = 0;
extern "C" int ivh_set_attn_kernel(int choice) {
  IVH_REQUIRE(choice >= 0 && choice <= 2, "ivh_set_attn_kernel: choice must be 0 (auto), 1 (16x16x32) or 2 (32x32x16)");
  g_attn_impl = choice;
  return 0;
}

static int attn_check(const AttnArgs& a) {
  IVH_REQUIRE(a.q && a.k && a.v, "flash_attn: null q/k/v");
  IVH_REQUIRE(a.B > 0 && a.H > 0 && a.Lq > 0 && a.Lk > 0, "flash_attn: empty problem B=%d H=%d Lq=%d Lk=%d", a.B, a.H, a.Lq, a.Lk);
  IVH_REQUIRE(a.hd > 0 && a.hd % 8 == 0 && a.hd <= 128, "flash_attn: head dim %d not supported (multiple of 8, <= 128)", a.hd);
  IVH_REQUIRE(a.sb % 8 == 0 && a.sl % 8 == 0 && a.sh % 8 == 0 && a.qsb % 8 == 0 && a.qsl % 8 == 0 && a.qsh % 8 == 0,
              "flash_attn: strides must be multiples of 8 elements");
  IVH_REQUIRE(((uintptr_t)a.q % 16) == 0 && ((uintptr_t)a.k % 16) == 0 && ((uintptr_t)a.v % 16) == 0, "flash_attn: q/k/v must be 16-byte aligned");
  IVH_REQUIRE(a.H <= 65535 && a.B <= 65535, "flash_attn: B, H must be <= 65535");
  return 0;
}

static int drop_cfg(float p, uint32_t seed, DropCfg* d) {
  IVH_REQUIRE(p >= 0.0f && p < 1.0f, "flash_attn dropout: p = %f outside [0, 1)", (double)p);
  const double t = (double)p * 4294967296.0;
  d->thresh = (unsigned)(t > 4294967295.0 ? 4294967295.0 : t);
  d->inv_keep = 1.0f / (1.0f - p);
  d->seed = seed;
  d->epoch = ivh_host::dropout_epoch();
  return 0;
}

// one workgroup per `rows` rows of a (b, h) slice
static long attn_wgs(const AttnArgs& a, int L, int rows) { return (long)((L + rows - 1) / rows) * a.H * a.B; }

// ---- routes: which kernel(s) a call runs, on what grid.  They launch nothing and dereference nothing; the entry points and ivh_attn_debug_route
// call these two and nothing else decides.
// Dropout on the probabilities (the *_dropout entry points) exists on the 16x16x32 kernels at head dims <= 64 only: the text tower's.
// nb_dev (the *_dyn entry points, ABI 2): int32 in HBM, the number of clips that exist -- the launch is sized for B, workgroups of clips at or past
// *nb_dev leave at once and none of their outputs is written (DropPath skipping: the kept clips of a branch are compacted to the front).  Needs
// the 32x32 forward / dQ kernel; either dK/dV kernel takes it.
static int route_attn_fwd(const AttnArgs& a, AttnRoute* r) {
  const char* name = a.dropout ? "flash_attn_fwd_dropout" : "flash_attn_fwd";
  if (attn_check(a)) return -1;
  IVH_REQUIRE(a.out && ((uintptr_t)a.out % 8) == 0 && a.ob % 4 == 0 && a.ol % 4 == 0 && a.oh % 4 == 0, "%s: bad out", name);
  const int hdp = attn_hdp(a.hd);
  const bool mid = hdp == 96;                             // the measurement variants below are built for 64 < hd <= 96 only
  AttnLaunch& l = r->launch[0];
  r->n = 1;
  l = AttnLaunch{16, ATTN_FWD, hdp, 0, (unsigned)attn_wgs(a, a.Lq, 64 * ATTN_FWD_QW), 256, 0, name};
  if (a.dropout) {
    DropCfg d;
    IVH_REQUIRE(a.hd <= 64, "flash_attn_fwd_dropout: built for head dims <= 64 (got %d)", a.hd);
    l.flags = ATTN_DROP;
    return drop_cfg(a.p_drop, a.seed, &d);
  }
  const bool ok32 = ((uintptr_t)a.out % 16) == 0 && attn32_supported(a);
  IVH_REQUIRE(g_attn_impl != 2 || ok32, "flash_attn_fwd: the 32x32 kernel was requested but does not support these strides / sizes");
  IVH_REQUIRE(!a.nb_dev || (ok32 && g_attn_impl != 1), "flash_attn_fwd_dyn: a device-side clip count needs the 32x32 kernels, which do not support this layout");
  if (g_attn_impl == 1 || !ok32) return 0;
  const Attn32Switches sw = attn32_switches();
  const int pp = sw.pingpong;
  if (pp >= 1 && pp <= 5 && (mid || !sw.stamps)) {        // two wave groups one phase apart; with a stamp buffer only where the stamping build exists
    l = AttnLaunch{32, ATTN_FWD2, hdp, 0, (unsigned)attn_wgs(a, a.Lq, 256), 512, 0, "flash_attn_fwd (32x32, two wave groups)"};
    if (sw.stamps) {                                      // segment stamps of workgroup 0, waves 0 and 4: [2][256] (tools/probes/attn_pp_stamps.py)
      IVH_REQUIRE(sw.stamp_rows >= 128, "flash_attn_fwd: the two-group stamp buffer holds 2 x 256 uint64");
      l.flags = ATTN_STAMP | (pp >= 4 ? ATTN_NP : 0);
      l.what = "flash_attn_fwd (32x32, two wave groups, stamps)";
    } else if (mid && pp >= 4) {                          // unpacked softmax arithmetic (5: + raised priority)
      l.flags = ATTN_NP | (pp == 5 ? ATTN_PRIO : 0);
      l.what = "flash_attn_fwd (32x32, two wave groups, unpacked softmax)";
    } else if (mid && pp == 3) {                          // groups = even / odd waves
      l.flags = ATTN_GSEL;
      l.what = "flash_attn_fwd (32x32, two wave groups, alternating)";
    } else {                                              // 1: plain, 2: MFMA segments at raised priority; 3 / 4 / 5 outside (64, 96] are 1
      l.flags = pp == 2 ? ATTN_PRIO : 0;
    }
    return 0;
  }
  const long wgs = attn_wgs(a, a.Lq, 128);
  l = AttnLaunch{32, ATTN_FWD, hdp, 0, (unsigned)wgs, 256, 0, "flash_attn_fwd (32x32)"};
  if (pp == 7 && mid && !sw.stamps) {                     // the shipped kernel at two waves per SIMD
    l.flags = ATTN_NP2;
    l.what = "flash_attn_fwd (32x32, two waves per SIMD)";
  } else if (pp == 6 && mid && !sw.stamps) {              // the one-group kernel with unpacked softmax arithmetic, whatever IVH_ATTN_NOPK says
    l.flags = ATTN_NP;
    l.what = "flash_attn_fwd (32x32, unpacked softmax)";
  } else {                                                // the shipped route: unpacked unless switched off; IVH_ATTN_DEFER=1 is packed outside (64, 96]
    if (sw.defer && sw.unpacked && mid) l.what = "flash_attn_fwd (32x32, deferred rescale)";
    l.flags = sw.defer ? (ATTN_DEFER | (sw.unpacked && mid ? ATTN_NP : 0)) : (sw.unpacked ? ATTN_NP : 0);
    if (sw.stamps) {                                      // this kernel writes 4 stamps per workgroup of the WHOLE grid, under every ping-pong mode
      IVH_REQUIRE(wgs <= sw.stamp_rows, "flash_attn_fwd: the stamp buffer holds %ld workgroups", sw.stamp_rows);
      l.flags |= ATTN_STAMP;
    }
  }
  return 0;
}

// dQ first: its prologue computes delta = <dO, O> per query row and leaves it in `delta` for the dK/dV kernel that follows
static int route_attn_bwd(const AttnArgs& a, AttnRoute* r) {
  const char* name = a.dropout ? "flash_attn_bwd_dropout" : "flash_attn_bwd";
  if (attn_check(a)) return -1;
  IVH_REQUIRE(a.out && a.dout && a.lse && a.delta && a.dq && a.dk && a.dv, "%s: null argument", name);
  IVH_REQUIRE(a.ob % 8 == 0 && a.ol % 8 == 0 && a.oh % 8 == 0 && ((uintptr_t)a.out % 16) == 0 && ((uintptr_t)a.dout % 16) == 0, "%s: out/dout alignment", name);
  IVH_REQUIRE(a.dsb % 4 == 0 && a.dsl % 4 == 0 && a.dsh % 4 == 0 && a.dqb % 4 == 0 && a.dql % 4 == 0 && a.dqh % 4 == 0, "%s: dq/dk/dv strides must be multiples of 4", name);
  const int hdp = attn_hdp(a.hd);
  AttnLaunch &dq = r->launch[0], &dkdv = r->launch[1];
  r->n = 2;
  dq = AttnLaunch{16, ATTN_DQ, hdp, 0, (unsigned)attn_wgs(a, a.Lq, 64), 256, 0, name};
  dkdv = AttnLaunch{16, ATTN_DKDV, hdp, 0, (unsigned)attn_wgs(a, a.Lk, 64), 256, 0, name};
  if (a.dropout) {
    DropCfg d;
    IVH_REQUIRE(a.hd <= 64, "flash_attn_bwd_dropout: built for head dims <= 64 (got %d)", a.hd);
    dq.flags = dkdv.flags = ATTN_DROP;
    return drop_cfg(a.p_drop, a.seed, &d);
  }
  const bool al16 = ((uintptr_t)a.dq % 16) == 0 && ((uintptr_t)a.dk % 16) == 0 && ((uintptr_t)a.dv % 16) == 0 && a.dqb % 8 == 0 && a.dql % 8 == 0 && a.dqh % 8 == 0 &&
                    a.dsb % 8 == 0 && a.dsl % 8 == 0 && a.dsh % 8 == 0;
  const bool ok32 = al16 && attn32_supported(a);
  IVH_REQUIRE(g_attn_impl != 2 || ok32, "flash_attn_bwd: the 32x32 kernels were requested but do not support these strides / sizes");
  const bool use32 = g_attn_impl != 1 && ok32;
  IVH_REQUIRE(!a.nb_dev || use32, "flash_attn_bwd_dyn: a device-side clip count needs the 32x32 dQ kernel, which does not support this layout");
  if (!use32) return 0;
  const int np = attn32_switches().unpacked ? ATTN_NP : 0;
  dq = AttnLaunch{32, ATTN_DQ, hdp, np, (unsigned)attn_wgs(a, a.Lq, 128), 256, 0, "flash_attn_bwd dq (32x32)"};
  const int lds = attn32_dkdv_lds_bytes(a.Lq, a.hd);      // 0: head dims above 96 (the 32x32 kernel would spill) and very long Lq stay on the 16x16 dK/dV kernel
  if (lds > 0) dkdv = AttnLaunch{32, ATTN_DKDV, hdp, np, (unsigned)attn_wgs(a, a.Lk, 128), 256, (unsigned)lds, "flash_attn_bwd dkdv (32x32)"};
  return 0;
}

// ---- launches.  Every 16x16x32 instantiation that exists, once: taking the address instantiates the kernel, and a launch whose key has no row
// is an error, never another flavour.  The 32x32 table is attn32_launch's (flash_attn32.hip).
struct Attn16Row { int kind, hdp, flags; void* fn; };
#define A16_ROWS(hdp, drop)                                                                                                                  \
  {ATTN_FWD, hdp, (drop) ? ATTN_DROP : 0, (void*)&attn_fwd_kernel<hdp, drop>}, {ATTN_DQ, hdp, (drop) ? ATTN_DROP : 0, (void*)&attn_bwd_dq_kernel<hdp, drop>}, \
      {ATTN_DKDV, hdp, (drop) ? ATTN_DROP : 0, (void*)&attn_bwd_dkdv_kernel<hdp, drop>}
static const Attn16Row attn16_table[] = {A16_ROWS(64, false), A16_ROWS(96, false), A16_ROWS(128, false), A16_ROWS(64, true)};
#undef A16_ROWS

static int attn_launch(const AttnArgs& a, const AttnLaunch& l) {
  if (l.family == 32) return attn32_launch(a, l);
  void* fn = nullptr;
  for (const Attn16Row& row : attn16_table)
    if (row.kind == l.kind && row.hdp == l.hdp && row.flags == l.flags) fn = row.fn;
  IVH_REQUIRE(fn, "%s: the 16x16 attention kernel of kind %d, HDP %d, flags 0x%x is not built", l.what, l.kind, l.hdp, l.flags);
  DropCfg d{0u, 1.0f, 0u};
  if (a.dropout && drop_cfg(a.p_drop, a.seed, &d)) return -1;
  const dim3 grid(l.grid, 1, 1), block(l.block);
  hipStream_t s = (hipStream_t)a.stream;
  switch (l.kind) {
    case ATTN_FWD:
      hipLaunchKernelGGL(reinterpret_cast<decltype(&attn_fwd_kernel<64>)>(fn), grid, block, l.lds, s, a.q, a.qsb, a.qsl, a.qsh, a.k, a.v, a.sb, a.sl, a.sh,
                         a.out, a.ob, a.ol, a.oh, a.lse, a.H, a.Lq, a.Lk, a.hd, a.scale, a.kv_len, d);
      break;
    case ATTN_DQ:
      hipLaunchKernelGGL(reinterpret_cast<decltype(&attn_bwd_dq_kernel<64>)>(fn), grid, block, l.lds, s, a.q, a.qsb, a.qsl, a.qsh, a.k, a.v, a.sb, a.sl, a.sh,
                         a.out, a.dout, a.ob, a.ol, a.oh, a.lse, a.delta, a.dq, a.dqb, a.dql, a.dqh, a.H, a.Lq, a.Lk, a.hd, a.scale, a.kv_len, d);
      break;
    default:
      hipLaunchKernelGGL(reinterpret_cast<decltype(&attn_bwd_dkdv_kernel<64>)>(fn), grid, block, l.lds, s, a.q, a.qsb, a.qsl, a.qsh, a.k, a.v, a.sb, a.sl, a.sh,
                         a.dout, a.ob, a.ol, a.oh, a.lse, a.delta, a.dk, a.dv, a.dsb, a.dsl, a.dsh, a.H, a.Lq, a.Lk, a.hd, a.scale, a.kv_len, d, a.nb_dev);
  }
  return check_launch(l.what);
}

static int attn_fwd(const AttnArgs& a) {
  AttnRoute r;
  return route_attn_fwd(a, &r) ? -1 : attn_launch(a, r.launch[0]);
}
static int attn_bwd(const AttnArgs& a) {
  AttnRoute r;
  if (route_attn_bwd(a, &r) || attn_launch(a, r.launch[0])) return -1;
  return attn_launch(a, r.launch[1]);
}

// ---- the C ABI (include/internvideo_hip.h, which this file includes: a list that drifts from the declaration does not compile).  The three
// flavours of a direction share its parameters up to kv_len; each is a thin wrapper that fills AttnArgs.
#define ATTN_FWD_PARAMS                                                                                                                   \
  const uint16_t *q, int64_t qsb, int64_t qsl, int64_t qsh, const uint16_t *k, const uint16_t *v, int64_t sb, int64_t sl, int64_t sh, uint16_t *out, \
      int64_t ob, int64_t ol, int64_t oh, float *lse, int B, int H, int Lq, int Lk, int hd, float scale, const int32_t *kv_len
#define ATTN_FWD_NAMES q, qsb, qsl, qsh, k, v, sb, sl, sh, out, ob, ol, oh, lse, B, H, Lq, Lk, hd, scale, kv_len
#define ATTN_BWD_PARAMS                                                                                                                   \
  const uint16_t *q, int64_t qsb, int64_t qsl, int64_t qsh, const uint16_t *k, const uint16_t *v, int64_t sb, int64_t sl, int64_t sh, const uint16_t *out, \
      const uint16_t *dout, int64_t ob, int64_t ol, int64_t oh, const float *lse, float *delta, uint16_t *dq, int64_t dqb, int64_t dql, int64_t dqh,      \
      uint16_t *dk, uint16_t *dv, int64_t dsb, int64_t dsl, int64_t dsh, int B, int H, int Lq, int Lk, int hd, float scale, const int32_t *kv_len
#define ATTN_BWD_NAMES q, qsb, qsl, qsh, k, v, sb, sl, sh, out, dout, ob, ol, oh, lse, delta, dq, dqb, dql, dqh, dk, dv, dsb, dsl, dsh, B, H, Lq, Lk, hd, scale, kv_len
static AttnArgs attn_fwd_args(ATTN_FWD_PARAMS, void* stream) {
  AttnArgs a = attn_args(q, qsb, qsl, qsh, k, v, sb, sl, sh, ob, ol, oh, B, H, Lq, Lk, hd, scale, kv_len, stream);
  a.out = out; a.lse = lse;
  return a;
}
static AttnArgs attn_bwd_args(ATTN_BWD_PARAMS, void* stream) {
  AttnArgs a = attn_args(q, qsb, qsl, qsh, k, v, sb, sl, sh, ob, ol, oh, B, H, Lq, Lk, hd, scale, kv_len, stream);
  a.out = const_cast<uint16_t*>(out); a.dout = dout; a.lse = const_cast<float*>(lse); a.delta = delta;
  a.dq = dq; a.dqb = dqb; a.dql = dql; a.dqh = dqh; a.dk = dk; a.dv = dv; a.dsb = dsb; a.dsl = dsl; a.dsh = dsh;
  return a;
}
static int attn_run(AttnArgs a, bool bwd, const int32_t* nb_dev, bool dropout, float p_drop, uint32_t seed) {
  a.nb_dev = nb_dev; a.dropout = dropout; a.p_drop = p_drop; a.seed = seed;
  return bwd ? attn_bwd(a) : attn_fwd(a);
}
extern "C" int ivh_flash_attn_fwd(ATTN_FWD_PARAMS, void* stream) { return attn_run(attn_fwd_args(ATTN_FWD_NAMES, stream), false, nullptr, false, 0.0f, 0u); }
extern "C" int ivh_flash_attn_bwd(ATTN_BWD_PARAMS, void* stream) { return attn_run(attn_bwd_args(ATTN_BWD_NAMES, stream), true, nullptr, false, 0.0f, 0u); }
extern "C" int ivh_flash_attn_fwd_dyn(ATTN_FWD_PARAMS, const int32_t* nb_dev, void* stream) {
  return attn_run(attn_fwd_args(ATTN_FWD_NAMES, stream), false, nb_dev, false, 0.0f, 0u);
}
extern "C" int ivh_flash_attn_bwd_dyn(ATTN_BWD_PARAMS, const int32_t* nb_dev, void* stream) {
  return attn_run(attn_bwd_args(ATTN_BWD_NAMES, stream), true, nb_dev, false, 0.0f, 0u);
}
// dropout on the probabilities: the drop probability and the seed of the counter-based mask; the same (p, seed) must be given to both directions
extern "C" int ivh_flash_attn_fwd_dropout(ATTN_FWD_PARAMS, float p_drop, uint32_t seed, void* stream) {
  return attn_run(attn_fwd_args(ATTN_FWD_NAMES, stream), false, nullptr, true, p_drop, seed);
}
extern "C" int ivh_flash_attn_bwd_dropout(ATTN_BWD_PARAMS, float p_drop, uint32_t seed, void* stream) {
  return attn_run(attn_bwd_args(ATTN_BWD_NAMES, stream), true, nullptr, true, p_drop, seed);
}
#undef ATTN_BWD_NAMES
#undef ATTN_BWD_PARAMS
#undef ATTN_FWD_NAMES
#undef ATTN_FWD_PARAMS

// ---- ivh_attn_debug_route (include/internvideo_hip_debug.h): the routes above, seen from outside.  Host logic only.
extern "C" int ivh_attn_debug_route(int bwd, int dropout, const uint64_t* addr7, const int64_t* strides15, int B, int H, int Lq, int Lk, int hd,
                                    int has_nb_dev, int* out16) {
  static float present_f;                                 // stands for the pointers the route only tests for NULL
  static int32_t present_i;
  const int64_t* st = strides15;
  const auto at = [&](int i) { return reinterpret_cast<uint16_t*>((uintptr_t)addr7[i]); };
  AttnArgs a = bwd ? attn_bwd_args(at(0), st[0], st[1], st[2], at(1), at(2), st[3], st[4], st[5], at(3), at(3), st[6], st[7], st[8], &present_f, &present_f, at(4), st[9],
                                   st[10], st[11], at(5), at(6), st[12], st[13], st[14], B, H, Lq, Lk, hd, 1.0f, nullptr, nullptr)
                   : attn_fwd_args(at(0), st[0], st[1], st[2], at(1), at(2), st[3], st[4], st[5], at(3), st[6], st[7], st[8], &present_f, B, H, Lq, Lk, hd, 1.0f, nullptr, nullptr);
  a.nb_dev = has_nb_dev ? &present_i : nullptr;
  a.dropout = dropout != 0;
  AttnRoute r;
  if (bwd ? route_attn_bwd(a, &r) : route_attn_fwd(a, &r)) return 0;
  for (int i = 0; i < r.n; ++i) {
    const AttnLaunch& l = r.launch[i];
    const int row[8] = {l.family, l.kind, l.hdp, l.flags, (int)l.grid, (int)l.block, (int)l.lds, 0};
    for (int j = 0; j < 8; ++j) out16[8 * i + j] = row[j];
  }
  return r.n;
}
