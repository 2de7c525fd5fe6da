/* internvideo_hip_debug.h -- measurement hooks and hardware probes of libinternvideo_hip.so.
 *
 * NOT part of the drop-in contract: include/internvideo_hip.h is what a reference-side binding binds; nothing here is
 * needed to run the path.  These entry points exist for tools/ (timelines, K-loop ablations, A/B switches, counter calibration) and for
 * the tests that pin the hardware semantics the kernels rely on (tests/test_kernels_gpu.py).  Process-wide switches, not thread-safe.
 */
#ifndef INTERNVIDEO_HIP_DEBUG_H
#define INTERNVIDEO_HIP_DEBUG_H
#include "internvideo_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* measurement aids for the 256x256 kernel (tools/bench_gemm.py): stagger = start-up skew unit (-1 = automatic, 0 = off),
 * skip_stores != 0 drops the C / preact stores (results are then NOT written). */
int ivh_gemm256_debug(int stagger, int skip_stores);
/* device buffer of 128 uint64 (or NULL): workgroup 0 records s_memtime stamps (4 per tile: K loop start, K loop end, DMA wait done,
 * epilogue end) for wave 0 ([0..63]) and wave 4 ([64..127]) */
int ivh_gemm256_debug_stamps(void* buf_128_u64);
int ivh_gemm256_debug_max_wg(int n);            /* cap the persistent grid (0 = one workgroup per CU) */
int ivh_gemm256_debug_sched(int sched);         /* K-loop schedule: 0 = two-group ping-pong, 1 = rolling (gemm256.hip) */
/* measurement aid: buf = device array of rows x 4 uint64 that receives wave 0's shader-clock stamps (entry, loop start, loop end, exit) of every
 * forward workgroup of the 32x32x16 attention kernel launched while it is set (tools/attn_timeline.py); NULL switches it off */
int ivh_attn32_debug_stamps(void* buf, int64_t rows);
int ivh_gemm256_debug_split(int on);           /* 0 = never split the tail round along K (A/B, tests); default 1 */
/* half-width tiles of the 256x256 kernel (ivh_gemm256_half_plan in internvideo_hip.h): 0 = off (A/B, tests), 1 = on, a workgroup's half tile
 * runs between its whole tiles (default), 2 = on, half tiles last */
int ivh_gemm256_debug_half(int on);
/* Host logic only (no device needed): the ten template arguments {a_kc, b_kc, epi, grouped, dbg, sched, fp8, split, half, dyn} of the
 * gemm256_kernel instantiation the launchers would run for *d on `cap` workgroups (0 = the device's CUs, 256 without a device), chosen by the
 * function the launchers themselves call.  mode 0 = the bf16 launch, 1 = the e4m3 launch as ivh_gemm_fp8 calls it under its default kernel
 * choice (size test on for a count-free descriptor), n >= 2 = the grouped launch of d[0 .. n).  Returns 1, or 0 when the launcher would refuse
 * the descriptor or hand it over to the 128x128 kernel (out10 is then not written). */
int ivh_gemm256_debug_route(const ivh_gemm_desc* d, int mode, int cap, int* out10);
/* Host logic only (no device needed, nothing dereferenced): the kernel one of the six ivh_rmsnorm_add_* entry points would launch, chosen by the
 * route function the entry points themselves call (norms.hip).  bwd: 0 forward, 1 backward.  flavour: 0 = ivh_rmsnorm_add_{fwd,bwd}, 1 = *_bf16res,
 * 2 / 3 = *_skip with res_bf16 = 0 / 1.  `set`: bit i = the entry's i-th POINTER argument (stream excluded) is non-NULL, counted over the _skip
 * entry's argument list -- forward: res_in, branch, gamma, rowscale, w, res_out, y, rstd, branch_slot, y_slot; backward: dy, dres_out, res_out,
 * rstd, w, branch, gamma, rowscale, dres_in, dbranch, dw_part, dgamma_part, dbias_part, dres_extra, y_slot, branch_slot.  Bits of arguments the
 * flavour's entry does not take (the slot maps outside _skip, dres_extra on flavour 0) are ignored.
 * Returns 1 and out9 = {b16, nch_t, wpr, rows, extra, skip, res_bf16, grid, shmem_bytes}: b16 = 0 is rmsnorm_add_{fwd,bwd}_kernel<nch_t, wpr,
 * float | bf16_t by res_bf16, skip> (rows = 0), b16 = 1 is rmsnorm_add_bwd_b16_kernel<nch_t, rows, extra, skip> (wpr = 0); extra = dres_extra is
 * passed; grid workgroups of 256 threads with shmem_bytes of dynamic LDS.  Returns 0, with ivh_last_error set and out9 untouched, when the
 * entry point would refuse the call. */
int ivh_rmsnorm_add_debug_route(int bwd, int flavour, unsigned set, int M, int D, int rows_per_sample, int* out9);
/* Host logic only (no device needed, nothing dereferenced): the launches one of the six ivh_flash_attn_* entry points would make, chosen by the
 * route functions the entry points themselves call (flash_attn.hip), under the process's ivh_set_attn_kernel / ivh_probe_attn32_* / stamp-buffer /
 * IVH_ATTN_* state.  bwd: 0 forward, 1 backward.  dropout != 0: the *_dropout entry (its probability taken as valid).  addr7 = the ADDRESSES
 * {q, k, v, out, dq, dk, dv}, only tested for NULL and alignment (the forward reads the first four; dout counts as out's address, lse and delta as
 * present); strides15 = {qsb, qsl, qsh, sb, sl, sh, ob, ol, oh, dqb, dql, dqh, dsb, dsl, dsh}; has_nb_dev != 0: the *_dyn entry with a clip count.
 * Returns the number of launches (1 forward; 2 backward: dQ, then dK/dV) and 8 ints per launch in out16: {family 16 | 32 (the MFMA shape of the
 * kernel file), kind, HDP, flags, grid.x, block, dynamic LDS bytes, 0}.  kind: 0 forward (attn_fwd_kernel / attn32_fwd*_kernel), 1 dQ, 2 dK/dV,
 * 3 the forward as two wave groups (attn32pp_fwd*_kernel).  flags: 1 DROP, 2 DEFER, 4 NP (the *_np_kernel builds), 8 NP2 (attn32_fwd_np2_kernel),
 * 16 PRIO, 32 GSEL, 64 STAMP (the stamp buffer is handed to the kernel; a template argument of the two-group kernels only).  Returns 0, with
 * ivh_last_error set and out16 untouched, when the entry point would refuse the call. */
int ivh_attn_debug_route(int bwd, int dropout, const uint64_t* addr7, const int64_t* strides15, int B, int H, int Lq, int Lk, int hd, int has_nb_dev,
                         int* out16);
int ivh_gemm256_debug_ablate(int mode);       /* K-loop ablation of the plain NT kernel: 0 off, 1 no MFMA, 2 no LDS-DMA, 3 no fragment reads (garbage results) */

/* probes used by tests/test_hw_probe.py to pin the hardware semantics the kernels rely on */
int ivh_probe_tr16(const uint16_t* in_4x16x4, uint16_t* out_64x4, void* stream);
int ivh_probe_mfma16(const uint16_t* a16x32, const uint16_t* b16x32, float* c16x16, void* stream);
int ivh_probe_mfma32(const uint16_t* a32x16, const uint16_t* b32x16, float* c32x32, void* stream);   /* c[i][j] = sum_k a[i][k] b[j][k], 32x32x16 layout */
/* known-rate MFMA stream (counter calibration, tools/pmc_mfma.py): `workgroups` x 4 waves x iters x 8 MFMAs 32x32x16 bf16 = 32768 FLOP each */
int ivh_probe_mfma_rate(int iters, int workgroups, float* sink, void* stream);
/* the same stream on either bf16 MFMA shape (0: 32x32x16, 1: 16x16x32; 262144 FLOP per wave and iteration both ways), 1 or 2 waves per SIMD */
int ivh_probe_mfma_rate2(int shape, int waves_per_simd, int iters, int workgroups, float* sink, void* stream);

/* a bounded number of CUs kept busy with memory traffic: `workgroups` x 256 threads copy `bytes` (multiple of 16) src -> dst.  bench.py runs it on a
 * side stream beside the training step with the wire bytes of an 8-GPU gradient all-reduce to price what collective kernels cost the step
 * (`comm_contention`): the part of the scaling prediction that one GPU can measure. */
int ivh_probe_cu_hog(const void* src, void* dst, int64_t bytes, int workgroups, void* stream);

/* round-5 prototype of the q/k-norm fusion (flash_attn32.hip, QKN): the 32x32 forward kernel on UN-normalised q, k with their per-token rstd
 * (rq, rk: fp32 [B * L]) and wqk = q_norm.weight * k_norm.weight (fp32 [H * hd]): Q scaled at its load, a per-key factor on the scores.
 * 64 < hd <= 96, Lq == Lk <= 512.  tools/probes/attn_qkn_fusion_probe.py prices it against qk_rmsnorm_fwd + the shipped kernel. */
int ivh_probe_attn32_fwd_qkn(const uint16_t* q, int64_t qsb, int64_t qsl, int64_t qsh, const uint16_t* k, const uint16_t* v, int64_t sb, int64_t sl, int64_t sh,
                             uint16_t* out, int64_t ob, int64_t ol, int64_t oh, float* lse, int B, int H, int Lq, int Lk, int hd, float scale,
                             const float* rq, const float* rk, const float* wqk, void* stream);

/* round-6 measurement switch (flash_attn32.hip, attn32pp_fwd_kernel): the forward as 8-wave workgroups whose two wave groups run one segment apart
 * (MFMA segment of one beside the softmax segment of the other).  0 = off (default; also the environment variable IVH_ATTN_PP read once),
 * 1 = on, 2 = on with the MFMA segments at raised wave priority, 3 = groups of even / odd waves, 4 / 5 = 1 / 2 without packed fp32 instructions,
 * 6 = the one-group kernel without packed fp32 instructions, 7 = the same at two waves per SIMD.  tools/bench_attn.py --pingpong prices it against the shipped kernel. */
int ivh_probe_attn32_pingpong(int mode);

/* round-6 switch: the three 32x32 attention kernels compiled with (0) or without (1, the default; environment IVH_ATTN_NOPK=0 selects 0) the packed fp32
 * instructions.  v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 of one wave do not run beside another wave's MFMAs on the same SIMD
 * (tools/probes/mfma_valu_mix.hip); results are bit-identical either way. */
int ivh_probe_attn32_unpacked(int on);

#ifdef __cplusplus
}
#endif
#endif
