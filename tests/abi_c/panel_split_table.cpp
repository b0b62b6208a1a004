// Prints the split-K table of csrc/gsmvi_panel_split.h: one line "items nchunks tune_panel_kc num_cu kc cpw" per combination
// (tests/test_panel_split_cpu.py compares it with a restatement of the three call sites it replaced).  Host only, no GPU.
#include <cstdio>

#include "gsmvi_panel_split.h"

int main() {
    const int items[] = {1, 2, 3, 16, 32, 48, 64, 128, 256, 257, 512, 1024};
    const int cus[] = {256, 64};
    for (int it : items)
        for (int nchunks = 1; nchunks <= 64; ++nchunks)
            for (int tune = 0; tune <= 9; ++tune)
                for (int cu : cus) {
                    const gsmvi_panel_split s = gsmvi_panel_split_k(it, nchunks, tune, cu, 8);
                    std::printf("%d %d %d %d %d %d\n", it, nchunks, tune, cu, s.kc, s.cpw);
                }
    return 0;
}
