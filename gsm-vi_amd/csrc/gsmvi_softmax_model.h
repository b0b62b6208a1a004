// The model block of the batched softmax entry points (gsmvi_softmax_batched.hip: score and density;
// gsmvi_softmax_laplace_batched.hip: Hessian and Newton step; gsmvi_psis_loo_softmax_batched.hip: PSIS-LOO;
// gsmvi_softmax_predict_batched.hip: the predictive; DESIGN.md section 9, "The softmax model block"): K multinomial logit
// regressions of one (rows, C, P), D = (C - 1) P <= 64.  One copy of what the entries share around their kernels: the model's
// fields, its shape rule and argument checks, its four read-only arrays in the overlap table, and on the device the padded row
// length, the MFMA chain of one class and the per-problem prologue of a kernel (valid rows, prior precision).  The counterpart of
// gsmvi_glm_model.h.  The kernels keep their own argument blocks (their layouts differ), so the device helpers take scalars.
#pragma once
#include "gsmvi_common.h"
#include "gsmvi_batched.h"
#include <cstddef>

// What every entry point builds from its arguments.  The predictive's M is its N and its labels may be null; the leave-one-out and
// the predictive have no prior (lam = 0).
struct sm_model {
    long long K, N;
    int C, P, D;                // classes, features, (C - 1) P (0 until the shape is checked: sm_model_of)
    const double* A;            // (K, N, P)
    const int* labels;          // (K, N)
    const int* counts;          // (K) valid rows, clamped to 0 .. N (null: N)
    double lam;                 // the prior precision of every problem ...
    const double* lam_dev;      // ... or (K) per-problem values on the device (null: `lam`)
};

// C >= 2 and 1 <= (C - 1) P <= 64, without forming a product that could overflow
static inline bool sm_shape_ok(int C, int P) { return C >= 2 && P >= 1 && C - 1 <= GB_MAX_D && P <= GB_MAX_D && (C - 1) * P <= GB_MAX_D; }

static inline sm_model sm_model_of(int64_t K, int64_t N, int C, int P, const double* A, const int* labels, const int* counts,
                                   double lam = 0.0, const double* lam_dev = nullptr) {
    return {K, N, C, P, sm_shape_ok(C, P) ? (C - 1) * P : 0, A, labels, counts, lam, lam_dev};
}

// Pp = 4 ceil(P / 4): the columns of a row of A that feeds the 16 x 16 x 4 MFMA class by class
__host__ __device__ inline int sm_pp(int P) { return ((P + 3) >> 2) << 2; }

// eta_c of the lane's four (draw, row) pairs: the MFMA chain of class c.  px points at the lane's row of the X tile (rows as in
// memory, class-major) plus kq, pb at its row of the A tile plus kq; a k position 4 j + kq >= P feeds 0.0 from the X side and loads
// nothing, so a padded position is 0 x 0 and no LDS word outside the row's D entries is read.
__device__ __forceinline__ v4d sm_eta(const double* px, const double* pb, int c, int P, int Pp, int kq) {
    const double* pa = px + c * P;
    v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < Pp; j += 4) acc = GSMVI_MFMA_F64(j + kq < P ? pa[j] : 0.0, pb[j], acc);
    return acc;
}

// s = sum_c exp(eta_c - m) as 1 + rest, and log s without the rounding of s.  A term e = exp(eta_c - m) is exactly 1 for a class
// that attains m and below 1 for every other, so floor(e) tells the two apart without a comparison: the terms below 1 are summed
// in class order (rest), the ones counted (nt >= 1), and rest + (nt - 1) is s - 1 with the relative error of a sum of positive
// terms.  log(s) alone returns 0 where rest < eps / 2 (the winning class ahead by more than 1 / eps), where the definition's log s
// is rest; sm_log_s adds what the rounding of s = 1 + rest dropped, d = rest - (s - 1) (exact while rest <= 1), as the first-order
// term d / s, with 2 - s for 1 / s below s = 2 (the error, d (s - 1)^2 / s, stays under 0.4 eps of log s) and nothing from s = 2 on
// (d / s <= eps / 2 next to log s >= 0.69): log1p(rest) to two eps, at the cost of log and six operations.
// k_softmax_batched, k_psis_loo_softmax_batched and k_softmax_predict_batched sum this way; k_softmax_laplace_batched has its own
// rest (it needs c*, the first class that attains m, for 1 - p) and shares sm_log_s.
__device__ __forceinline__ void sm_add_term(double& rest, double& nt, double e) {
    const double f = floor(e);
    rest += e - f;
    nt += f;
}

__device__ __forceinline__ double sm_rest(double rest, double nt) { return rest + (nt - 1.0); }

__device__ __forceinline__ double sm_log_s(double rest, double s) {
    const double d = rest - (s - 1.0);
    return log(s) + (s < 2.0 ? d * (2.0 - s) : 0.0);
}

// the rows of problem k that count: counts[k] clamped to 0 .. N (null: N)
__device__ __forceinline__ long long sm_rows_of(const int* counts, long long k, long long N) {
    if (!counts) return N;
    const long long c = counts[k];
    return c < 0 ? 0 : (c > N ? N : c);
}

// what a packed kernel needs of problem k before its sweep: the rows that count and lam_k.  A slot that is not `valid` (a tail
// slot, a frozen problem) has no rows that count, so it loads nothing of A_k.  k_softmax_batched is the exception: it keeps these
// statements written out, because built on this function its six instantiations got other instructions (the same registers,
// LDS and occupancy) and two of nine timed shapes came out slower than the parent's run-to-run spread allows.
struct sm_problem {
    long long nk;
    double lam;
};

__device__ __forceinline__ sm_problem sm_problem_of(const int* counts, double lam, const double* lam_dev, long long N, long long k,
                                                    bool valid) {
    sm_problem p = {0, 0.0};
    if (valid) {
        p.nk = sm_rows_of(counts, k, N);
        p.lam = lam_dev ? lam_dev[k] : lam;
    }
    return p;
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// The checks every softmax entry point makes of its model, in this order: C, then P and D; K; the rows (`rows` names them in the
// message: "N", or "M" for the predictive); and for a packed entry "K N D" and the prior.  `packed`: the entries whose kernels pack
// gb_nt(D) threads per problem and have a prior (score, Hessian, step) follow gb_check_shape's K rule; the two that run one
// workgroup per tile of rows (leave-one-out, predictive) take K in [1, 2^24 - 1] and carry overflow checks of their own.
static inline int sm_check_model(const char* fn, const sm_model& m, bool packed, const char* rows) {
    char msg[64];
    if (m.C < 2) return gb_bad(fn, "C must be at least 2");
    if (!sm_shape_ok(m.C, m.P)) return gb_bad(fn, "P must be at least 1 and D = (C - 1) P in [1, 64]");
    if (packed) {
        if (int st = gb_check_shape(fn, m.K, m.D, gb_ppw)) return st;
    } else if (m.K < 1 || m.K > 16777215)
        return gb_bad(fn, "K must be in [1, 2^24 - 1]");
    if (m.N < 1) {
        snprintf(msg, sizeof msg, "%s must be at least 1", rows);
        return gb_bad(fn, msg);
    }
    if (packed) {
        if (m.N > (INT64_MAX / 8 / m.D) / m.K) return gb_bad(fn, "K N D is too large");
        if (!m.lam_dev && !(m.lam >= 0.0 && m.lam < __builtin_huge_val())) return gb_bad(fn, "prior_prec must be finite and >= 0");
    }
    return GSMVI_OK;
}

// gb_check_overlaps over the model's four read-only arrays followed by the entry point's own
template <size_t NOWN>
static inline int gb_check_overlaps(const char* fn, const sm_model& m, const gb_arr (&own)[NOWN]) {
    const size_t nn = (size_t)m.K * m.N;
    gb_arr all[4 + NOWN] = {{m.A, nn * m.P * 8, "A", GB_RD},
                            {m.labels, nn * 4, "labels", GB_RD},
                            {m.counts, (size_t)m.K * 4, "counts_dev", GB_RD},
                            {m.lam_dev, (size_t)m.K * 8, "prior_prec_dev", GB_RD}};
    for (size_t i = 0; i < NOWN; ++i) all[4 + i] = own[i];
    return gb_check_overlaps(fn, all, all + 4 + NOWN);
}
