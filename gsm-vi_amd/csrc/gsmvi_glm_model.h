// The model block of the batched GLM entry points (gsmvi_logistic_batched.hip: score and density; gsmvi_laplace_batched.hip:
// Hessian and Newton step; gsmvi_glm_predict_batched.hip: the predictive): K generalised linear models of
// one (N, D), D <= 64.  One copy of what the entries share around their kernels: the model's fields, its argument checks, its
// six read-only arrays in the overlap table, the dispatch on the family, and the per-problem prologue of a kernel (valid rows,
// prior precision, noise precision).  The numerics of the families are in gsmvi_glm_link.h.
#pragma once
#include "gsmvi_batched.h"
#include "gsmvi_glm_link.h"
#include <cstddef>
#include <type_traits>

// What every entry point builds from its arguments, and the first member of lp_args and gp_args (k_logistic_batched keeps an
// argument block of its own, see lb_args).  The predictive's M is its N; its y may be null and it has no prior (lam = 0).
struct glm_model {
    long long K, N;
    int D;
    const double* A;            // (K, N, D)
    const double* y;            // (K, N)
    const double* offset;       // (K, N) added to eta, or null
    const int* counts;          // (K) valid rows, clamped to 0 .. N (null: N)
    double lam;                 // the prior precision of every problem ...
    const double* lam_dev;      // ... or (K) per-problem values on the device (null: `lam`)
    double tau;                 // gaussian family: the noise precision of every problem ...
    const double* tau_dev;      // ... or (K) per-problem values on the device (null: `tau`)
};

// Dp = 16 ceil(D / 16): the columns of a tile that feeds the 16 x 16 x 4 MFMA
__host__ __device__ inline int glm_dp(int D) { return ((D + 15) >> 4) << 4; }

// what a kernel needs of problem k before its sweep: the rows that count, lam_k and tau_k
struct glm_problem {
    long long nk;
    double lam, tau;
};

// A slot that is not `valid` (a tail slot, a frozen problem) has no rows that count, so it loads nothing of A_k.  tau is read
// only by the gaussian family.  (m by value: by reference, two kernels come out of the compiler with other register counts)
template <int FAM>
__device__ __forceinline__ glm_problem glm_problem_of(const glm_model m, long long k, bool valid) {
    glm_problem p = {0, 0.0, 1.0};
    if (valid) {
        p.nk = m.N;
        if (m.counts) {
            const long long c = m.counts[k];
            p.nk = c < 0 ? 0 : (c > m.N ? m.N : c);
        }
        p.lam = m.lam_dev ? m.lam_dev[k] : m.lam;
        if (FAM == LB_GAUSSIAN) p.tau = m.tau_dev ? m.tau_dev[k] : m.tau;
    }
    return p;
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// The checks every GLM entry point makes of its model: the shape, the family and its noise precision, and (has_prior) the prior.
// `rows` names the row count in the messages: "N", or "M" for the predictive.
static inline int glm_check_model(const char* fn, const glm_model& m, int family, const char* rows, bool has_prior) {
    char msg[64];
    if (int st = gb_check_shape(fn, m.K, m.D, gb_ppw)) return st;
    if (m.N < 1) {
        snprintf(msg, sizeof msg, "%s must be at least 1", rows);
        return gb_bad(fn, msg);
    }
    if (m.N > (INT64_MAX / 8 / m.D) / m.K) {
        snprintf(msg, sizeof msg, "K %s D is too large", rows);
        return gb_bad(fn, msg);
    }
    if (family < GSMVI_GLM_LOGISTIC || family > GSMVI_GLM_GAUSSIAN)
        return gb_bad(fn, "family must be one of GSMVI_GLM_LOGISTIC .. GSMVI_GLM_GAUSSIAN");
    if (has_prior && !m.lam_dev && !(m.lam >= 0.0 && m.lam < __builtin_huge_val()))
        return gb_bad(fn, "prior_prec must be finite and >= 0");
    if (family == GSMVI_GLM_GAUSSIAN) {
        if (!m.tau_dev && !(m.tau > 0.0 && m.tau < __builtin_huge_val())) return gb_bad(fn, "noise_prec must be finite and > 0");
    } else if (m.tau_dev || m.tau != 1.0)
        return gb_bad(fn, "noise_prec is the gaussian family's: give 1.0 and NULL for any other");
    return GSMVI_OK;
}

// gb_check_overlaps over the model's six read-only arrays followed by the entry point's own
template <size_t NOWN>
static inline int gb_check_overlaps(const char* fn, const glm_model& m, const gb_arr (&own)[NOWN]) {
    const size_t ny = (size_t)m.K * m.N * 8, nk = (size_t)m.K * 8;
    gb_arr all[6 + NOWN] = {{m.A, ny * m.D, "A", GB_RD},
                            {m.y, ny, "y", GB_RD},
                            {m.offset, ny, "offset", GB_RD},
                            {m.counts, (size_t)m.K * 4, "counts_dev", GB_RD},
                            {m.tau_dev, nk, "noise_prec_dev", GB_RD},
                            {m.lam_dev, nk, "prior_prec_dev", GB_RD}};
    for (size_t i = 0; i < NOWN; ++i) all[6 + i] = own[i];
    return gb_check_overlaps(fn, all, all + 6 + NOWN);
}

// f(integral_constant<int, LB_...>) for a checked `family`: the template instantiation of a launch
template <typename F>
static inline void glm_for_family(int family, F&& f) {
    switch (family) {
        case GSMVI_GLM_LOGISTIC: f(std::integral_constant<int, LB_LOGISTIC>{}); break;
        case GSMVI_GLM_POISSON: f(std::integral_constant<int, LB_POISSON>{}); break;
        case GSMVI_GLM_PROBIT: f(std::integral_constant<int, LB_PROBIT>{}); break;
        default: f(std::integral_constant<int, LB_GAUSSIAN>{}); break;
    }
}
