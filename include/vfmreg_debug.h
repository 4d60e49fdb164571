/*
 * vfmreg_debug.h -- measurement hooks and tuning switches of libvfmreg_hip.so used by bench.py, tools/ and tests/.
 *
 * NOT part of the drop-in contract (include/vfmreg.h, SURVEY.md 8 B.5: "no global state except the last-error string").
 * Everything declared here either keeps state outside the caller's buffers or synchronises the device:
 *   - vfm_prof_*      THREAD-LOCAL, one shot: vfm_prof_arm() stores two HIP events in thread-local storage of the calling
 *                     thread; the next coarse launch issued FROM THAT THREAD (vfm_match_search_coarse* / vfm_match_ip_top1* /
 *                     vfm_match_search_prepared / vfm_match_search_probe_half) records them around its dominant kernel on the
 *                     stream it is launched on and clears the slot.  No other thread and no later search sees them.
 *   - (until round 5 this header also held vfm_debug_set_*: PROCESS-GLOBAL A/B switches.  They are gone: kernel policy is a caller-owned
 *     vfm_config_t bound per thread -- include/vfmreg.h, vfm_config_* -- and vfmreg/_lib.py keeps the old names as Python functions that
 *     set the calling thread's config, for the tools.)
 *   - vfm_debug_match_stats / vfm_debug_i8_rows / vfm_debug_mx6_rows / vfm_debug_ransac_state  read-backs for tests; they synchronise the device.
 *   - vfm_debug_search_plan / vfm_debug_coarse_plan / vfm_debug_prepare_plan / vfm_debug_vit_plan  read the calling thread's vfm_config and nothing
 *                     else; host memory only.
 *   - vfm_debug_l2_narrow_slices  host arithmetic only; vfm_debug_l2_narrow_evals  reads a workspace's counters and synchronises the device.
 *   - vfm_debug_last_coarse_kernel / vfm_debug_coarse_kernel_names  THREAD-LOCAL like vfm_prof_*: which instantiation of the coarse kernels
 *                     the last search issued FROM THE CALLING THREAD launched, and the names of all of them; host memory only.
 */
#ifndef VFMREG_DEBUG_H
#define VFMREG_DEBUG_H

#include "vfmreg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* HIP events around the dominant kernel (the MFMA coarse pass of the top-1 search), recorded on the stream that kernel is
 * launched on.  vfm_prof_arm() applies to the NEXT search issued from the calling thread (one shot, thread-local).
 * vfm_prof_elapsed_ms() waits for `stop`. */
int vfm_prof_events_create(void **start, void **stop);
int vfm_prof_arm(void *start, void *stop);
int vfm_prof_elapsed_ms(void *start, void *stop, float *ms_host);
int vfm_prof_events_destroy(void *start, void *stop);

/* tests: which coarse kernel ran.  Every instantiation of the kernels of csrc/match_coarse_*.hip has a name spelled from its template arguments
 * ("i8q2<12,top2=0,low=0,fused=0>", "mx6q2<3,FUSE,low=0,img=6,ring=5,T=4,NS=3>", "pipe<24,sparse>+seed": the sparse fp16 kernel launched with
 * seed units), and a launch notes it per thread.  vfm_debug_last_coarse_kernel: the name noted last by the calling thread -- the
 * Euclidean entry points launch one kernel per direction, the reverse direction last -- or "" if it has launched none.
 * vfm_debug_coarse_kernel_names: every name a launch can note, sorted, separated by '\n'; the list is generated from the same lines of
 * csrc/match_internal.h that instantiate the kernels.  Both write a NUL-terminated string to buf_host[cap] (VFM_EINVAL if it does not
 * fit) and do not touch the device. */
int vfm_debug_last_coarse_kernel(char *buf_host, int cap);
int vfm_debug_coarse_kernel_names(char *buf_host, int cap);

/* tests / callers' policy: what a search of these arguments would do under the calling thread's vfm_config, resolved by the same function
 * the search entry points use -- `records` as passed to them (a kind, VFM_RECORDS_NO_I8 beside it or not), gated: the gated family or not.
 * One line of text to buf_host[cap]:
 *     pass=<f16-dense|f16-sparse|int8|fp6> kind=<the VFM_RECORDS_* value the search runs as, after every fallback; 2 for an fp16 pass>
 *     half=<0|1> fused=<0|1> top2=<0|1> pilot=<0|1> bins=<0|1: the chunk-major rescan runs> no_i8=<0|1>
 *     finish=<the kernels of the finish stage in launch order, separated by ','>
 * A combination the search refuses fails here with the same error.  Host memory only: no device is touched. */
int vfm_debug_search_plan(int records, int d, int64_t n, int64_t m, int gated, char *buf_host, int cap);

/* tests / tools: the launch of that search's coarse pass, resolved by the function the search itself calls once (csrc/match_internal.h,
 * resolve_coarse, behind resolve_search).  inner_product: 0 for the fp16 pass of the Euclidean entry points (d: their padded K); row_bias:
 * that pass at K = 640 / 768, which adds a bias per map row; compute_units: of the device asked about, 0: the current device's.  One line
 * of text to buf_host[cap]:
 *     kernel=<the name vfm_debug_last_coarse_kernel reports after the launch> nqb=<query blocks> nslices=<map slices>
 *     seed=<workgroups of the seed round at the head of the grid> block=<threads> lds=<bytes of dynamic LDS> tune=<CoarseArgs::tune>
 * The grid is seed + nqb x nslices workgroups.  A combination the search refuses fails here with the same error.  Host memory only. */
int vfm_debug_coarse_plan(int records, int d, int64_t n, int64_t m, int gated, int inner_product, int row_bias, int compute_units,
                          char *buf_host, int cap);

/* tests / tools: what a preparation would do under the calling thread's vfm_config, resolved by the same function the entry points use.
 * entry: which of them is asked about -- the six exported ones, and the two forms the library uses inside vfm_match_mutual_l2 (one operand,
 * the int8 image alone) and the ungated vfm_match_ip_top1; schedule / dtype1 / dtype2: as passed to the entry (0 where it takes none);
 * rows2 = 0 for the one-operand entries; zero: the search workspace ranges of vfm_match_prepare2_gated_z ride along.  One line of text to
 * buf_host[cap]:
 *     images=<the images written, ','-separated: f16, i8, fp6 or fp6h (the first d / 2 columns only)>
 *     kernels=<the launches in order, ','-separated, each instantiation spelled from its template arguments: prep_chunk_kernel<false,2,true,8>,
 *              prep_once_kernel<384,half,persist,noi8>, ...>
 *     grid=<workgroups of the first launch: group (one per 128 rows) | tile (per 32 rows) | cu (one per compute unit) | 2cu-stream (two per
 *           compute unit of the stream's mask) | n>
 *     zero=<none | inside (the preparation kernel clears the ranges) | behind (prep_zero_kernel does)>
 * A combination the entry refuses fails here with the same error.  Host memory only: no device is touched. */
enum vfm_debug_prepare_entry {
    VFM_PREP_ENTRY_PREPARE = 0,   /* vfm_match_prepare */
    VFM_PREP_ENTRY_PREPARE2,      /* vfm_match_prepare2 */
    VFM_PREP_ENTRY_GATED,         /* vfm_match_prepare2_gated (and the gated vfm_match_ip_top1_gated) */
    VFM_PREP_ENTRY_GATED_P,       /* vfm_match_prepare2_gated_p */
    VFM_PREP_ENTRY_GATED_Z,       /* vfm_match_prepare2_gated_z */
    VFM_PREP_ENTRY_GATED_T,       /* vfm_match_prepare2_gated_t */
    VFM_PREP_ENTRY_PERM,          /* inside vfm_match_mutual_l2 */
    VFM_PREP_ENTRY_ONESHOT        /* inside vfm_match_ip_top1 */
};
int vfm_debug_prepare_plan(int entry, int schedule, int d, int64_t rows1, int dtype1, int64_t rows2, int dtype2, int zero, char *buf_host,
                           int cap);

/* counters of the last FAST search that used workspace `ws` (candidate histogram, refined / fallback queries;
 * see csrc/match_finish.hip).  out64_host: HOST int32[64].  Synchronises the device. */
int vfm_debug_match_stats(void *ws, int64_t n, int64_t m, int32_t *out64_host);
/* tools: wall-clock stamps (100 MHz) workgroup 0 of the one-launch VoxelDownsample kernel took behind each of its grid-wide barriers
 * during the last vfm_voxel_robin in `ws` (n as at that call; recorded while vfm_debug_set_voxel_small(101) is in force, 100 = off);
 * out_host: HOST int64[32], [31] = number of stamps.  Synchronises the device. */
int vfm_debug_voxel_trace(void *ws, int64_t n, int64_t *out_host);
/* tests: the int8 image of a prepared operand (d = 256, 384) unpacked on the host -- q8_host[rows][d], and per row the
 * quantisation step of its 128-row group, its residual norm E and the group's maximum E.  Synchronises the device. */
int vfm_debug_i8_rows(const void *prepared, int64_t rows, int d, int8_t *q8_host, float *step_host,
                      float *err_host, float *gerr_host);
/* tests: the fp6 image of an operand prepared with VFM_PREPARE_MX6 (d = 256, 384), dequantised on the host -- v6_host[rows][d]
 * (code value x block scale), and per row the image's residual norm E (arithmetic slack included) and its group's maximum.
 * Synchronises the device. */
int vfm_debug_mx6_rows(const void *prepared, int64_t rows, int d, float *v6_host, float *err_host, float *gerr_host);
/* tests: the same image's residual norm over the first d / 2 columns (the bound of the half-width fp6 kinds) and its group maximum */
int vfm_debug_mx6_half_err(const void *prepared, int64_t rows, int d, float *errh_host, float *gerrh_host);
/* tests / bench: what the last vfm_ransac_corr in `ws` (same c_max, n_iter) did: out_host[0] = hypotheses scored in fp64 from the candidate
 * list, [1] = the list overflowed (every hypothesis scored in fp64), [2] = the point-wise fp32 pass was needed.  Synchronises. */
int vfm_debug_ransac_counts(const void *ws, int64_t c_max, int32_t n_iter, int32_t *out_host);
/* tests: everything the last vfm_ransac_corr in `ws` (same c_max, n_iter) left there, copied to HOST buffers; any of them may be NULL.
 * Reads only; synchronises the device.
 *   n_lo / n_hi / r_lo / r_hi [n_iter]   the bounds of every hypothesis (n_hi < 0: degenerate sample, or fewer than 3 correspondences),
 *                                        from the point-wise fp32 pass if sel[3] is set, else from the closed-form moment pass
 *   sel [4]                              F (max n_lo), count, overflow, unsure; *rstar = R* (min r_hi over n_lo = n_hi = F; +inf if none).
 *                                        count: the hypotheses the bounds could not rule out, NOT clamped to the list's capacity
 *   list [VFM_DEBUG_RANSAC_CAND_MAX]     the first min(count, CAND_MAX) survivors in the order they were appended (no particular order)
 *   fit / rmse / hyp [CAND_MAX + nblocks], nblocks = (n_iter + 63) / 64: the exact fp64 scores, hyp = -1 for an empty slot (fit = rmse = 0:
 *                                        nothing scored there, a degenerate sample, or a hypothesis without a single inlier)
 * Which slots a call fills depends on the chain ("ransac_fused"):
 *   2 (default), 0   list: yes.  Slot k < CAND_MAX: the score of list[k] for k < count, empty for k >= count -- and ALL CAND_MAX slots are
 *                    empty when the list overflowed.  Slot CAND_MAX + b: empty unless the list overflowed; then the best of hypotheses
 *                    [64 b, 64 b + 64) under (fitness desc, rmse asc, id asc), every one of them scored.
 *   1                no list (`list` and the slots k < CAND_MAX are not written: they hold what an earlier call left), no capacity and so
 *                    never an overflow.  Slot CAND_MAX + b: the best of the SURVIVORS among hypotheses [64 b, 64 b + 64), empty if none.
 *   "ransac_exact_only": slots [0, nblocks) hold the per-block best of all hypotheses; bounds, sel and list are not written. */
#define VFM_DEBUG_RANSAC_CAND_MAX 2048
int vfm_debug_ransac_state(const void *ws, int64_t c_max, int32_t n_iter, int32_t *n_lo_host, int32_t *n_hi_host, double *r_lo_host,
                           double *r_hi_host, int32_t *sel_host, double *rstar_host, int32_t *list_host, double *fit_host,
                           double *rmse_host, int32_t *hyp_host);

/* tests: where vfm_vit_forward(cfg, ..., B, ...) keeps its buffers inside the caller's workspace, in the order x (fp32 [M][dim] residual
 * stream), a (fp16 fragment tiles: im2col, then the attention output), xh (fp16 fragment copy of x), stats (fp32 [M][dim / 32][2]), h (fp16
 * fragment tiles [M][mlp_dim]), q, k (fp16 fragments per (image, head): [Tp][64]), vt (per (image, head): [64][Tp]); M = B * Tp, Tp = tokens
 * padded to 32.  offsets_host / bytes_host: HOST int64[8]; bytes = the extent up to the next buffer (padding to 256 bytes included).  Computed
 * by the forward's own carving routine.  After a forward the buffers hold what the LAST block left: q / k / vt are not written under
 * "vit_fused_qkv", h is not written under "vit_fused_mlp".  Does not touch the device. */
int vfm_debug_vit_workspace_layout(const vfm_vit_config *cfg, int B, int64_t *offsets_host, int64_t *bytes_host);

/* tests / tools: what vfm_vit_forward(cfg, ..., B images W pixels wide ...) would launch under the calling thread's vfm_config, resolved by
 * the function the forward itself calls once (csrc/vit_plan.h, resolve_vit).  compute_units: of the device asked about, 0: the current
 * device's.  One line of text to buf_host[cap]:
 *     pre=.. patch=.. qkv=.. att=.. proj=.. fc1=.. fc2=..   each stage's launch as <kernel>@<workgroups>x<threads>+<bytes of dynamic LDS>, the
 *              kernel an instantiation spelled from its template arguments (vit_gemm_lds_kernel<RESID,2,3>, vit_attention_lds_kernel<11>, ...);
 *              a block's launches are those of every layer; "-": the stage is inside the kernel before it (att in vit_qkv_attention_kernel,
 *              fc2 in vit_mlp_kernel)
 *     launches=<kernel launches of the whole forward> trace=<the one stage whose launch gets "vit_trace_buffer" | none>
 * A model or batch the forward refuses fails here with the same error.  Host memory only.
 * The "vit_*" keys of vfm_config_set beside "vit_fused_qkv" / "vit_fused_mlp" (include/vfmreg.h); the same results under every value but "vit_hot_a":
 *   "vit_preprocess_patch"  1 (default): preprocessing by one workgroup per patch; 0: a thread per fragment unit
 *   "vit_xcd"               1 (default) / 0: a token tile's work on the workgroups of one XCD in every kernel, or not
 *   "vit_cfg_narrow", "vit_cfg_wide"  the direct GEMM kernel's wave tile and prefetch depth for N <= 512 / N > 512: 108 (default), 116, 208
 *   "vit_wpw"               waves per workgroup of the direct kernel: n > 0; 0 (default): one
 *   "vit_lds_min_wg"        the LDS-tiled GEMM from this many workgroups on: n > 0 (default 256); 0: never
 *   "vit_lds_shape"         its k-steps per stage x 10 + stages: 23 (default), 24, 25, 26, 42, 43
 *   "vit_wide_tile"         1: its residual GEMMs of 384 channels as one 128 x 384 tile per workgroup; 0 (default): 128 x 128
 *   "vit_hot_a"             timing experiment of the LDS-tiled kernel, WRONG RESULTS: bits 0 .. 3; 0 (default)
 *   "vit_att_lds_min"       attention with K / V^T through the LDS from this many images on: n > 0 (default 1); 0: never
 *   "vit_astat_min"         the token-stationary QKV / fc1 kernel from this many groups of 128 rows on: n > 0; 0 (default): where its rounds of
 *                           one workgroup per compute unit are full; -1: never
 *   "vit_astat_nw"          its waves per workgroup: 6, 8, 12, 16 where they divide the channel tiles, 112 = 12 with non-temporal stores; 0 (default): 12
 *   "vit_astat_two"         1 (default) / 0: two channel tiles per wave (eight waves) / one
 *   "vit_trace_fused"       which launch of a block gets the trace buffer: 0 (default) the token-stationary fc1, or else the LDS-tiled fc2;
 *                           1 vit_qkv_attention_kernel; 2 the LDS-tiled proj; 3 vit_mlp_kernel
 *   "vit_trace_buffer"      a device pointer (all 64 bits of the value) to the buffer that launch writes its per-workgroup stamps to; 0 (default): none */
int vfm_debug_vit_plan(const vfm_vit_config *cfg, int B, int W, int compute_units, char *buf_host, int cap);

/* VFM_MATCH_NARROW (csrc/match_l2_narrow.hip).  vfm_debug_l2_narrow_slices: the number of map slices the host rule gives a search of n
 * queries among m map rows (the grid is ceil(n / 256) query blocks x slices); 0 for n or m <= 0.  Host only, no device is touched.
 * vfm_debug_l2_narrow_evals: how many (query, map row) pairs the last vfm_match_mutual_l2(VFM_MATCH_NARROW) or vfm_match_mutual_pairs
 * (d <= 64) in workspace `ws` decided by the exact fp64 distance -- out2_host: HOST int64[2], [0] the a -> b direction, [1] the reverse
 * one (0 if it did not run).  Synchronises the device. */
int vfm_debug_l2_narrow_slices(int64_t n, int64_t m);
int vfm_debug_l2_narrow_evals(const void *ws, int64_t *out2_host);

#ifdef __cplusplus
}
#endif
#endif /* VFMREG_DEBUG_H */
