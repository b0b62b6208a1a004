/*
 * gsmvi_hip_debug.h -- diagnostic entry points (NOT part of the drop-in boundary of gsmvi_hip.h).  They are exported by
 * libgsmvi_hip_debug.so only -- the same objects linked with csrc/exports_debug.map -- never by the product library
 * libgsmvi_hip.so (its export list hides them and --gc-sections drops their host code).  Used by scripts/ (in-kernel
 * timelines, soaks); select the debug build with GSMVI_HIP_DEBUG_LIB=1 before importing gsmvi_amd.
 */
#ifndef GSMVI_HIP_DEBUG_H
#define GSMVI_HIP_DEBUG_H

#include "gsmvi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* Read back in-kernel s_memrealtime stamps: with the tuning knob "timeline" = 1 the first n words of the stamp buffer
 * ([kernel slot 0..3][512 workgroups][8 words]; workgroups beyond 512 write nothing), otherwise (knob "cov_dbg" bits
 * 16 / 128) the first n words of the panel-partial slab. */
int gsmvi_debug_read_stamps(gsmvi_ctx* ctx, unsigned long long* out, int n);
/* Read back a slice of the context workspace (region 0 panel slabs, 1 finished panels, 2 small matrices). */
int gsmvi_debug_read_workspace(gsmvi_ctx* ctx, int region, size_t offset, double* out, size_t n);
/* Device address of the region's base (0: panel partials, 1: finished panels, 2: small matrices), for in-place views. */
int gsmvi_debug_workspace_ptr(gsmvi_ctx* ctx, int region, double** out);
/* The one-workgroup n x n Cholesky kernels of the factor path's 2B x 2B chain (64 < n <= 128) on caller data: A (n x n, upper
 * triangle read) -> R (upper), and with_inverse != 0 also W = R^-T (lower) with the rank-revealing rule of the Gram matrix.
 * For soak / determinism scripts. */
int gsmvi_debug_chol128(void* stream, int n, int with_inverse, const double* A, double* R, double* W, int* info_dev);

/* Calibration for bench.py: a plain streaming copy of n doubles on `stream` (16 bytes per lane, non-temporal) -- the rate a
 * kernel that only moves bytes reaches on this box, the yardstick beside the 8 TB/s specification. */
int gsmvi_debug_stream_copy_f64(void* stream, double* dst, const double* src, size_t n);

/* The dynamic LDS bytes per workgroup, and the problems one workgroup holds, of a batched BaM launch at (D, B) (pad != 0: the
 * odd row strides of the default, pad = 0: the knob "bam_batched_pad" = 0).  Host arithmetic only, no device needed. */
int gsmvi_debug_bam_batched_lds(int D, int B, int pad, size_t* bytes, int* problems_per_workgroup);

/* The same for a batched ADVI launch at (D, B): mode 0 = gsmvi_advi_init_batched_f64, 1 = gsmvi_advi_step_batched_f64,
 * 2 = gsmvi_advi_cov_batched_f64 (B plays no part).  Host arithmetic only, no device needed. */
int gsmvi_debug_advi_batched_lds(int D, int B, int mode, size_t* bytes, int* problems_per_workgroup);

/* The same for a gsmvi_logistic_batched_f64 launch at (D, nc): want 1 = G alone, 2 = lp alone, 3 = both.  Host arithmetic only,
 * no device needed. */
int gsmvi_debug_logistic_batched_lds(int D, int nc, int want, size_t* bytes, int* problems_per_workgroup);

/* The same for a gsmvi_glm_batched_f64 launch of `family` (GSMVI_GLM_*) at (D, nc), with (has_offset != 0) or without an offset,
 * by the rule the launch itself uses: the tile of the offset (32 doubles per problem) is there with an offset and, for
 * GSMVI_GLM_POISSON, always.  Without the tile the figures are those of gsmvi_debug_logistic_batched_lds.  Host arithmetic only,
 * no device needed. */
int gsmvi_debug_glm_batched_lds(int D, int nc, int want, int family, int has_offset, size_t* bytes,
                                int* problems_per_workgroup);

/* The same for a gsmvi_glm_shared_batched_f64 launch of `family` at D (neither nc nor N plays a part: the one tile of A), and the
 * stacked rows of X one workgroup takes.  Host arithmetic only, no device needed. */
int gsmvi_debug_glm_shared_batched_lds(int D, int want, int family, size_t* bytes, int* rows_per_workgroup);

/* The same for a gsmvi_negbin_batched_f64 launch at (D = P + 1 in 2 .. 64, nc), with (has_offset != 0) or without an offset: at
 * most GB_LDS_MAX (76 KB: four problems of D = 16 with both outputs and an offset).  Host arithmetic only, no device needed. */
int gsmvi_debug_negbin_batched_lds(int D, int nc, int want, int has_offset, size_t* bytes, int* problems_per_workgroup);

/* The same for a gsmvi_ordinal_batched_f64 launch at (C >= 2, P >= 1, P + C - 1 <= 64, nc), with (has_offset != 0) or without an
 * offset: at most GB_LDS_MAX (113.1 KB: one problem of C = 64 with both outputs and an offset).  Host arithmetic only, no device
 * needed. */
int gsmvi_debug_ordinal_batched_lds(int C, int P, int nc, int want, int has_offset, size_t* bytes, int* problems_per_workgroup);

/* The same for a gsmvi_negbin_hessian_batched_f64 or gsmvi_negbin_laplace_step_batched_f64 launch at D = P + 1 in 2 .. 64 (both
 * request the same, with or without an offset): at most 64 KB, so no kernel attribute.  Host arithmetic only, no device needed. */
int gsmvi_debug_negbin_laplace_lds(int D, size_t* bytes, int* problems_per_workgroup);

/* The same for a gsmvi_ordinal_hessian_batched_f64 or gsmvi_ordinal_laplace_step_batched_f64 launch at D = P + C - 1 in 2 .. 64 (both
 * request the same, with or without an offset; the retry rule needs no LDS of its own): at most 64 KB, so no kernel attribute.
 * Host arithmetic only, no device needed. */
int gsmvi_debug_ordinal_laplace_lds(int D, size_t* bytes, int* problems_per_workgroup);

/* The same for a gsmvi_softmax_batched_f64 launch at (C, P, nc), and the rows of X one tile holds at (C, P) (the launch holds
 * min(nc, that) rows).  Host arithmetic only, no device needed. */
int gsmvi_debug_softmax_batched_lds(int C, int P, int nc, int want, size_t* bytes, int* problems_per_workgroup,
                                    int* x_rows_per_tile);

/* The same for a gsmvi_softmax_hessian_batched_f64 or gsmvi_softmax_laplace_step_batched_f64 launch at (C, P) (both request the
 * same: H aliases the sweep's tiles).  Host arithmetic only, no device needed. */
int gsmvi_debug_softmax_laplace_lds(int C, int P, size_t* bytes, int* problems_per_workgroup);

/* The same for a batched L-BFGS launch at D: mode 0 = gsmvi_lbfgs_step_batched_f64, 1 = gsmvi_lbfgs_hess_inv_batched_f64.  Host
 * arithmetic only, no device needed. */
int gsmvi_debug_lbfgs_batched_lds(int D, int mode, size_t* bytes, int* problems_per_workgroup);

/* The same for a gsmvi_pathfinder_propose_batched_f64 launch at D, and the rows of draws one tile holds (whatever M is).  Host
 * arithmetic only, no device needed. */
int gsmvi_debug_pathfinder_batched_lds(int D, size_t* bytes, int* problems_per_workgroup, int* tile_rows);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* GSMVI_HIP_DEBUG_H */
