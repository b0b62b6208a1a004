// How long does a wave wait for its kernel arguments, and does this machine's firmware preload them?  
//
// One kernel, two pointer and two integer arguments and a 256-byte by-value block behind them.  Thread 0 of every workgroup reads
// the shader clock (s_memtime) and the 100 MHz clock (s_memrealtime), each read waited for before the next instruction:
//   c0, c1   two reads back to back                       -> c1 - c0 = the cost of a read itself (subtracted below)
//   c2       behind an explicit scalar load of argument `a` (offset 0x10) and its wait
//                                                         -> one argument round trip if the line is not in the scalar cache
//   c3       behind a scalar load of the dword at OFF bytes into the block and its wait
//                                                         -> short when OFF shares a line with what has been fetched, a round trip
//                                                            when it does not: OFF = 0x20 .. 0x100 shows the line size
// Built twice by scripts/kernarg_probe.sh: plain, and with -mllvm -amdgpu-kernarg-preload-count=6 (`out`, `src`, `a`, `b` arrive in
// SGPRs; the compiler puts a compatibility prologue -- scalar loads of the same dwords and one wait -- in front of the kernel, and
// firmware that preloads enters behind it).  The prologue stands in front of the first instruction written here, so the clock cannot
// bracket it; what tells the two apart is c2: firmware that preloads skips the prologue, nothing has touched the argument line, and
// c2 - c1 is a full round trip as in the plain build; firmware that does not has just run the prologue's loads, and c2 - c1 is a
// scalar-cache hit.  `a + b` is stored so that the preloaded values are checked.
// The launches are replayed from a hipGraph, as bench.py replays the update: REPS graph launches of NL kernel nodes.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                              \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } \
    } while (0)

struct pad_block { int v[64]; };
constexpr int WORDS = 10;            // per workgroup: c0..c3, r0..r3 (100 MHz), a + b, the block's dword

__device__ __forceinline__ unsigned long long clk() {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}
__device__ __forceinline__ unsigned long long rclk() {
    unsigned long long t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}

template <int OFF>
__global__ __launch_bounds__(512) void k_probe(unsigned long long* out, const int* src, int a, int b, pad_block pad) {
    const char* ka = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
    const unsigned long long c0 = clk(), r0 = rclk();
    const unsigned long long c1 = clk(), r1 = rclk();
    int va, vp;
    asm volatile("s_load_dword %0, %1, 0x10\n\ts_waitcnt lgkmcnt(0)" : "=s"(va) : "s"(ka) : "memory");
    const unsigned long long c2 = clk(), r2 = rclk();
    asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(vp) : "s"(ka), "i"(0x18 + OFF) : "memory");
    const unsigned long long c3 = clk(), r3 = rclk();
    if (threadIdx.x == 0) {
        unsigned long long* o = out + (size_t)blockIdx.x * WORDS;
        o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
        o[4] = r0; o[5] = r1; o[6] = r2; o[7] = r3;
        o[8] = (unsigned long long)(unsigned)(a + b + src[0] + (va - a));     // = a + b + src[0]: checks the (preloaded) values
        o[9] = (unsigned long long)(unsigned)(vp - pad.v[OFF / 4]);           // = 0
    }
}

static double pct(std::vector<double> v, double p) {
    std::sort(v.begin(), v.end());
    return v[(size_t)(p * (v.size() - 1))];
}

template <int OFF>
static void run(hipStream_t st, unsigned long long* d_out, const int* d_src, int nwg) {
    constexpr int NL = 16, REPS = 8;
    pad_block pad;
    for (int i = 0; i < 64; ++i) pad.v[i] = 1000 + i;
    hipGraph_t g;
    hipGraphExec_t ge;
    CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeGlobal));
    for (int l = 0; l < NL; ++l)
        hipLaunchKernelGGL(k_probe<OFF>, dim3(nwg), dim3(512), 0, st, d_out + (size_t)l * nwg * WORDS, d_src, 40 + l, 2, pad);
    CHECK(hipStreamEndCapture(st, &g));
    CHECK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    std::vector<unsigned long long> h((size_t)NL * nwg * WORDS);
    std::vector<double> d_self, d_arg, d_off, r_arg, r_off;
    bool ok = true;
    for (int rep = 0; rep < REPS; ++rep) {
        CHECK(hipGraphLaunch(ge, st));
        CHECK(hipStreamSynchronize(st));
        CHECK(hipMemcpy(h.data(), d_out, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost));
        if (rep == 0) continue;                       // first replay: code and argument pages cold
        for (int l = 0; l < NL; ++l)
            for (int w = 0; w < nwg; ++w) {
                const unsigned long long* o = &h[((size_t)l * nwg + w) * WORDS];
                const double self = (double)(o[1] - o[0]);
                d_self.push_back(self);
                d_arg.push_back((double)(o[2] - o[1]) - self);
                d_off.push_back((double)(o[3] - o[2]) - self);
                r_arg.push_back((double)(o[6] - o[5]) - (double)(o[5] - o[4]));
                r_off.push_back((double)(o[7] - o[6]) - (double)(o[5] - o[4]));
                ok = ok && o[8] == (unsigned long long)(40 + l + 2 + 7) && o[9] == 0;
            }
    }
    printf("{\"off\": %d, \"values_ok\": %s, \"clock_read_cycles\": [%.0f, %.0f], \"arg_line_cycles\": [%.0f, %.0f], "
           "\"block_dword_cycles\": [%.0f, %.0f], \"arg_line_10ns\": [%.1f, %.1f], \"block_dword_10ns\": [%.1f, %.1f]}\n",
           OFF, ok ? "true" : "false", pct(d_self, 0.5), pct(d_self, 0.95), pct(d_arg, 0.5), pct(d_arg, 0.95), pct(d_off, 0.5),
           pct(d_off, 0.95), pct(r_arg, 0.5), pct(r_arg, 0.95), pct(r_off, 0.5), pct(r_off, 0.95));
    CHECK(hipGraphExecDestroy(ge));
    CHECK(hipGraphDestroy(g));
}

int main() {
    const int nwg = 256;
    hipStream_t st;
    CHECK(hipStreamCreate(&st));
    unsigned long long* d_out;
    int* d_src;
    CHECK(hipMalloc(&d_out, sizeof(unsigned long long) * 16 * nwg * WORDS));
    CHECK(hipMalloc(&d_src, sizeof(int)));
    const int seven = 7;
    CHECK(hipMemcpy(d_src, &seven, sizeof(int), hipMemcpyHostToDevice));
    // [median, p95] over the workgroups of 7 x 16 replayed launches; cycles of s_memtime, and units of 10 ns of s_memrealtime
    run<0x08>(st, d_out, d_src, nwg);     // block dword at kernarg offset 0x20: the line of `a` if lines are >= 64 B
    run<0x28>(st, d_out, d_src, nwg);     // 0x40
    run<0x68>(st, d_out, d_src, nwg);     // 0x80
    run<0xe8>(st, d_out, d_src, nwg);     // 0x100
    CHECK(hipFree(d_out));
    CHECK(hipFree(d_src));
    CHECK(hipStreamDestroy(st));
    return 0;
}
