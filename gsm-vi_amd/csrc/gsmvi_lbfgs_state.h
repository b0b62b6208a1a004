// The state of a batched L-BFGS minimisation (sc, ist, S, Y of gsmvi_lbfgs_step_batched_f64 in include/gsmvi_hip.h; DESIGN.md
// section 9, "Batched L-BFGS initialiser") and the dense inverse-Hessian estimate that its held pairs define: the layout, the
// ring-buffer test, the clamped read of the counters, and the recursion H <- (I - rho s y^T) H (I - rho y s^T) + rho s s^T.
// The layout and gl_held serve gsmvi_lbfgs_batched.hip and gsmvi_pathfinder_batched.hip; the functions below them serve
// k_pf_propose (the estimate from H_0 = gamma I at every accepted iterate).  k_lbfgs_step_batched (the clamp) and
// k_lbfgs_hess_inv_batched (the estimate from H_0 = I) keep the same statements inline, so a change here belongs there too.
#pragma once
#include "gsmvi_batched.h"

#define GL_M 10        // history length (scipy's maxcor)
#define GL_NSC 24      // doubles per problem in sc
#define GL_NIS 8       // ints per problem in ist
enum { GL_F = 0, GL_T = 1, GL_GD = 2, GL_SY = 4, GL_YY = 14 };   // sc: f, t, g.d, a spare, s.y and y.y of the ten slots
enum { GL_STATUS = 0, GL_NIT = 1, GL_NFEV = 2, GL_NLS = 3, GL_NP = 4, GL_HEAD = 5 };   // ist: .., pairs held, next slot, two spares

// is ring-buffer slot i one of the n pairs that end at head - 1
__device__ __forceinline__ bool gl_held(int i, int head, int n) {
    int o = i - (head - n);
    if (o >= GL_M) o -= GL_M;
    if (o < 0) o += GL_M;          // head - n >= -10
    return o < n;
}

// the pairs held and the next slot of the problem whose counters are `is`, clamped (an uploaded state cannot index outside the
// buffers)
__device__ __forceinline__ void gl_load_ring(const int* is, int& np, int& head) {
    np = is[GL_NP];
    head = is[GL_HEAD];
    np = np < 0 ? 0 : (np > GL_M ? GL_M : np);
    head = ((head % GL_M) + GL_M) % GL_M;
}

// The dense estimate of the problem of one workgroup slot, in two calls, so that the caller's other loads can follow the fill.
// All in the slot's LDS: H (D x D, row stride ld), Sl, Yl (10 x D each), u (D), lsy (10).
// gl_dense_fill, for a slot that is on (no barrier): Sl, Yl <- the held pairs of problem kk of S, Y (the ring buffers in global
// memory, (K, 10, D)), zeros elsewhere; H <- base I.
template <int NT>
__device__ __forceinline__ void gl_dense_fill(int D, int l, int ld, int np, int head, double base, const double* S, const double* Y,
                                              size_t kk, double* H, double* Sl, double* Yl) {
    const int DD = D * D;
    for (int e = l; e < GL_M * D; e += NT) {
        const bool h = gl_held(e / D, head, np);
        Sl[e] = h ? S[kk * GL_M * D + e] : 0.0;
        Yl[e] = h ? Y[kk * GL_M * D + e] : 0.0;
    }
    for (int e = l; e < DD; e += NT) {
        const int i = e / D, j = e - i * D;
        H[i * ld + j] = i == j ? base : 0.0;
    }
}

// gl_dense_rounds, for every slot (`on` is uniform in the slot; 2 + 2 x 10 barriers, the first publishes the fill and the last
// H): lsy[i] <- s_i . y_i summed in the order 0 .. D - 1; then over the held pairs, oldest to newest,
// H <- H - rho (s u^T + u s^T) + (rho^2 y.u + rho) s s^T with u = H y and rho = 1 / s.y: exactly symmetric ((i, j) and (j, i) come
// from the same products in the same order).
template <int NT>
__device__ __forceinline__ void gl_dense_rounds(bool on, int D, int l, int ld, int np, int head, double* H, const double* Sl,
                                                const double* Yl, double* u, double* lsy) {
    const int DD = D * D;
    __syncthreads();
    if (on && l < GL_M) {                                               // s.y of slot l, summed in the order 0 .. D - 1
        double acc = 0.0;
        for (int j = 0; j < D; ++j) acc += Sl[l * D + j] * Yl[l * D + j];
        lsy[l] = acc;
    }
    __syncthreads();
    for (int p = 0; p < GL_M; ++p) {                                    // oldest to newest; every slot runs all ten rounds
        const bool go = on && p < np;
        int i = head - np + p;
        if (i < 0) i += GL_M;
        const double* s = Sl + i * D;
        const double* y = Yl + i * D;
        if (go && l < D) {                                              // u = H y
            double acc = 0.0;
            for (int j = 0; j < D; ++j) acc += H[l * ld + j] * y[j];
            u[l] = acc;
        }
        __syncthreads();
        if (go) {
            const double rho = 1.0 / lsy[i];
            double yu = 0.0;                                            // every thread the same sum in the same order
            for (int j = 0; j < D; ++j) yu += y[j] * u[j];
            const double c = (rho * rho) * yu + rho;
            for (int e = l; e < DD; e += NT) {
                const int r = e / D, q = e - r * D;
                H[r * ld + q] = (H[r * ld + q] - rho * (s[r] * u[q] + u[r] * s[q])) + c * (s[r] * s[q]);
            }
        }
        __syncthreads();
    }
}
