// Split-K of the panel products: the one place that decides how many slabs a product leaves and how many chunks of the
// inner dimension each workgroup walks.  Host code without a HIP type in it: gsmvi_abi.hip is the only translation unit of
// the library that includes it, and tests/abi_c/panel_split_table.cpp prints its table on a machine without a GPU.
#pragma once

struct gsmvi_panel_split {
    int kc;    // slabs (the grid's y extent): every slab holds whole chunks, none is empty
    int cpw;   // chunks per workgroup
};

// items = workgroups of one slab (strips * zblocks), nchunks = chunks of the inner dimension (>= 1), tune_panel_kc > 0 = the
// wanted slab count (the "panel_kc" knob); otherwise two workgroups per CU are wanted.  The wanted count is clamped to
// [1, min(nchunks, max_kc)] (max_kc = GSMVI_MAX_KC: the slabs the workspace holds) and then lowered to the count that
// ceil(nchunks / kc) chunks per workgroup really fill.
static inline gsmvi_panel_split gsmvi_panel_split_k(int items, int nchunks, int tune_panel_kc, int num_cu, int max_kc) {
    int kc = tune_panel_kc > 0 ? tune_panel_kc : (2 * num_cu + items - 1) / items;
    if (kc > nchunks) kc = nchunks;
    if (kc > max_kc) kc = max_kc;
    if (kc < 1) kc = 1;
    gsmvi_panel_split s;
    s.cpw = (nchunks + kc - 1) / kc;
    s.kc = (nchunks + s.cpw - 1) / s.cpw;
    return s;
}
