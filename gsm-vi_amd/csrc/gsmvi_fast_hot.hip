// Entry points of the two-launch dense GSM update whose first load batch needs no kernel-argument fetch (round 15; knob
// "kernarg_preload").
//
// A workgroup cannot issue a vector load before the arguments that form its address have come through the scalar cache, which is
// cold at every kernel start.  gfx950 can deliver the leading dwords of the argument block in SGPRs with the wave (kernarg
// preload): the Makefile compiles THIS translation unit alone with -mllvm -amdgpu-kernarg-preload-count=14, and the entry points
// below begin with exactly what their first load batch takes -- pointers first, then the 32-bit values, 14 dwords, no struct
// (the compiler stops preloading at the first by-value struct).  The user-SGPR budget is 16: the kernarg pointer takes two.
// Everything else -- outputs, stamps, 1 / B -- follows the hot block and is fetched by ordinary scalar loads that nothing in
// front of the first vector loads waits for.  Firmware without the feature runs the compatibility prologue the compiler puts in
// front (the same values by one batch of scalar loads and one wait).
//
// The bodies are the ones of k_panel_fast<.., PART> and k_gsm_cov_sym<.., FROM_SLABS, .., QUAD> in gsmvi_fast.hip, one copy:
// the same instructions on the same values in the same order, so slabs, partial dots, mu and S are the bytes of the other entry
// points.  Covered: every product form of the route except whole-sample Qm ("panel_qm_whole"); of the covariance launch the quad
// map and the plain four-slab form (what the gated shapes run by default).  The launch helpers return false for the rest -- the
// A/B forms of the two-slab launch without the quads -- and the caller takes the entry points of gsmvi_fast.hip.
#define GSMVI_FAST_BODIES_ONLY
#include "gsmvi_fast.hip"

// Product: G, S0 (first batch), X, mu0 (the partial-dot loads behind it), their leading dimensions, D, the sample count and the
// chunks per workgroup = 14 dwords.  alpha = 1, no shift, no finished output: constants here.
template <int MT, int CHW, int STREAM>
__global__ __launch_bounds__(512) void k_panel_part_hot(const double* __restrict__ G, const double* __restrict__ S0, const double* X,
                                                        const double* mu0, int ldg, int lds0, int D, int nrows, int ldx,
                                                        int chunks_per_wg, double* Pp, unsigned long long* __restrict__ stamps,
                                                        double* Qg, double* Qm) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    gsmvi_panel_extras px;                     // (PART's arguments ride in free members: gsmvi_ctx.h)
    px.sj_src = X;
    px.sj_len = ldx;
    px.msl = mu0;
    px.sj_dst = Qg;
    px.mfin = Qm;
    panel_fast_body<MT, false, CHW, false, false, false, true, false, STREAM>(t0, D, nrows, G, ldg, nullptr, 1.0, S0, lds0, Pp, chunks_per_wg, D,
                                                                              stamps, nullptr, 0, nullptr, px);
}

// Covariance launch: the partial dots, the slabs, X, mu0 (first batch), S0 (the last loads of that batch), ldx, D, lds0 and one
// dword that holds B (low half) and the slab count (high half) = 14 dwords.  Qm = Qg + B * KC * strips and strips = D / 16
// (gsmvi_ctx.h: gsm_slab_src; the launch helper checks both), so neither is an argument.
struct gsm_cov_cold {                          // what no load of the first batch needs: fetched where it is first used
    double invB;
    double* S;
    double* mu_out;
    unsigned long long* stamps;
    int lds;
};

template <int SB, int KCT, bool FOLD, bool S0L, bool WT, bool QUAD, bool WST>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(!(WST && SB == 32) ? 4 : 2))) void k_gsm_cov_slabs_hot(
    const double* Qg, const double* Pp, const double* X, const double* __restrict__ mu0, const double* __restrict__ S0, int ldx, int D,
    int lds0, int b_kc, gsm_cov_cold cold) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    const int B = b_kc & 0xffff, KC = b_kc >> 16;
    gsm_slab_src fs;
    fs.X = X;
    fs.ldx = ldx;
    fs.Pp = Pp;
    fs.Qg = Qg;
    fs.KC = KC;
    fs.strips = D >> 4;
    fs.Qm = Qg + (size_t)B * KC * (D >> 4);
    gsm_cov_sym_body<SB, false, true, KCT, FOLD, S0L, WT, false, QUAD, WST>(t0, D, B, cold.invB, nullptr, 0, mu0, S0, lds0, cold.S, cold.lds, cold.mu_out, 0,
                                                                            cold.stamps, fs);
}

// ---- launch helpers: false = this form has no preloaded entry point (nothing was launched) --------------------------------------
// stream: the STREAM instance as gsmvi_launch_panel_fast_part chose it (2, 4; 0; -1 = the unstreamed code with its landing profile)
bool gsmvi_launch_panel_part_hot(hipStream_t st, hipEvent_t* ev, dim3 grid, int D, int B, const double* G, int ldg, const double* S0,
                                 int lds0, double* Pp, int chunks_per_wg, const double* X, int ldx, const double* mu0, double* Qg,
                                 double* Qm, int chw, int stream, unsigned long long* stamps) {
#define PH(MTV, CW, NS) GSMVI_LAUNCH((k_panel_part_hot<MTV, CW, NS>), grid, dim3(512), 0, st, ev, G, S0, X, mu0, ldg, lds0, D, B, ldx, \
                                     chunks_per_wg, Pp, stamps, Qg, Qm)
    if (chw == 512) {
        if (stream == 2) PH(1, 512, 2);
        else if (stream == 4) PH(1, 512, 4);
        else if (stream == -1) PH(1, 512, -1);
        else PH(1, 512, 0);
    } else if (chw == 256) {
        if (B == 16) PH(1, 256, 0);
        else if (B == 32) PH(2, 256, 0);
        else return false;
    } else return false;
#undef PH
    return true;
}

// grid, quad, fold: as gsmvi_launch_gsm_cov_sym_slabs chose them.  Covered: the quad map (both slab counts, both store paths) and
// the plain four-slab form without quads and fold -- what the gated shapes run by default.  (The folded four-slab form, reached with
// an explicit "panel_kc" at D = 1024 only, spills 12 bytes behind this entry point at B = 32: it keeps the one of gsmvi_fast.hip.)
bool gsmvi_launch_gsm_cov_slabs_hot(hipStream_t st, hipEvent_t* ev, dim3 grid, int D, int B, const gsm_slab_src& fs, const double* mu0,
                                    const double* S0, int lds0, double* S, int lds, double* mu_out, int kct, bool fold, bool quad,
                                    bool wave_store, unsigned long long* stamps) {
    if (fs.strips != D / 16 || fs.Qm != fs.Qg + (size_t)B * fs.KC * fs.strips || (B != 16 && B != 32)) return false;
    if (!quad && (kct != 4 || fold)) return false;
    gsm_cov_cold cold;
    cold.invB = 1.0 / (double)B;
    cold.S = S;
    cold.mu_out = mu_out;
    cold.stamps = stamps;
    cold.lds = lds;
#define CH(SBV, KV, FV, LV, WV, QV, SV)                                                                                             \
    GSMVI_LAUNCH((k_gsm_cov_slabs_hot<SBV, KV, FV, LV, WV, QV, SV>), grid, dim3(512), 0, st, ev, fs.Qg, fs.Pp, fs.X, mu0, S0, fs.ldx, D, \
                 lds0, B | (fs.KC << 16), cold)
#define CHD(SBV, KV, LV, WV) do { if (wave_store) CH(SBV, KV, false, LV, WV, true, true); else CH(SBV, KV, false, LV, WV, true, false); } while (0)
    if (!quad) { if (B == 16) CH(16, 4, false, false, false, false, false); else CH(32, 4, false, false, false, false, false); }
    else if (kct == 2) { if (B == 16) CHD(16, 2, true, true); else CHD(32, 2, true, true); }
    else { if (B == 16) CHD(16, 4, false, false); else CHD(32, 4, false, false); }
#undef CHD
#undef CH
    return true;
}
