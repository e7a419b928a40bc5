// Developer micro-test (GPU box): pins the semantics of the DPP row shifts the row-tree sums of dsim_core.hpp rely on
// (dsim_hip.hip: DevExec::row_from_above / row_from_below), of the row shifts by one and two quads and of the row folds of the
// quad body level's subtree sums (DevExec::odd_rows / upper_half), and of the row broadcast of the joint-space mat-vec
// (DevExec::row_matvec: row_newbcast:n, lane n of each 16-lane row to every lane of that row).  hipcc --offload-arch=gfx950 -O2 dpp_semantics.hip -o dpp_semantics
#include <hip/hip_runtime.h>
#include <cstdio>

template <int CTRL, bool BC> __device__ int dpp(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xf, 0xf, BC); }

__global__ void k(int* out) {
    const int lane = threadIdx.x;
    const int v = 100 + lane;
    out[0 * 64 + lane] = dpp<0x101, false>(-1, v);   // row_shl:1, old = -1, bound_ctrl off
    out[1 * 64 + lane] = dpp<0x111, false>(-1, v);   // row_shr:1
    out[2 * 64 + lane] = dpp<0x108, false>(-1, v);   // row_shl:8
    out[3 * 64 + lane] = dpp<0x101, true>(-1, v);    // row_shl:1, bound_ctrl on
    int r = -7;
    if (lane != 5) r = dpp<0x101, false>(-1, v);     // lane 5 disabled: what does lane 4 read?
    out[4 * 64 + lane] = r;
    out[5 * 64 + lane] = dpp<0x130, false>(-1, v);   // wave_shl:1
    out[6 * 64 + lane] = dpp<0x138, false>(-1, v);   // wave_shr:1
    out[7 * 64 + lane] = dpp<0x104, true>(-1, v);    // row_shl:4, bound_ctrl on: the next quad of the row, 0 in the row's last quad
    out[8 * 64 + lane] = dpp<0x108, true>(-1, v);    // row_shl:8, bound_ctrl on
    out[9 * 64 + lane] = __builtin_amdgcn_permlane16_swap(v, v, false, false)[1];    // expected: rows 0, 2 hold rows 1, 3 of v
    out[10 * 64 + lane] = __builtin_amdgcn_permlane32_swap(v, v, false, false)[1];   // expected: rows 0, 1 hold rows 2, 3 of v
    out[11 * 64 + lane] = dpp<0x150, false>(-1, v);  // row_newbcast:0: expected 100 in row 0, 116 in row 1, 132, 148
    out[12 * 64 + lane] = dpp<0x15d, false>(-1, v);  // row_newbcast:13: expected 113, 129, 145, 161
    // the instruction form the kernels use: acc = fma(x[lane n of the row], h, acc) with the broadcast on the operand, written
    // right behind the VALU instruction that produces x (the s_nop covers the two wait states).  x = 2 * v, h = lane, acc = 1000:
    // expected 1000 + 2 * (100 + 16 * row + 5) * lane, exact in fp32
    float x = (float)v, acc = 1000.f;
    const float h = (float)lane;
    x = x + x;
    asm volatile("s_nop 1\n\t"
                 "v_fmac_f32_dpp %0, %1, %2 row_newbcast:5 row_mask:0xf bank_mask:0xf" : "+v"(acc), "+v"(x) : "v"(h));
    out[13 * 64 + lane] = (int)acc;
    // a chain of two terms on one accumulator, as the mat-vec runs them: 1000 + 2 * (100 + 16 * row) * lane + 2 * (115 + 16 * row)
    float acc2 = 1000.f;
    const float one = 1.f;
    asm volatile("v_fmac_f32_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f32_dpp %0, %1, %3 row_newbcast:15 row_mask:0xf bank_mask:0xf" : "+v"(acc2) : "v"(x), "v"(h), "v"(one));
    out[14 * 64 + lane] = (int)acc2;
}

constexpr int NT = 15;

int main() {
    int* d;
    hipMalloc(&d, NT * 64 * 4);
    hipLaunchKernelGGL(k, 1, 64, 0, 0, d);
    int h[NT * 64];
    hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    const char* names[NT] = {"row_shl:1 old=-1 bc=0", "row_shr:1 old=-1 bc=0", "row_shl:8 old=-1 bc=0", "row_shl:1 old=-1 bc=1",
                             "row_shl:1, lane 5 disabled", "wave_shl:1", "wave_shr:1", "row_shl:4 old=-1 bc=1", "row_shl:8 old=-1 bc=1",
                             "permlane16_swap(v, v)[1]", "permlane32_swap(v, v)[1]", "row_newbcast:0 old=-1 bc=0", "row_newbcast:13 old=-1 bc=0",
                             "fmac_dpp row_newbcast:5", "fmac_dpp chain :0, :15"};
    for (int t = 0; t < NT; ++t) {
        printf("%-28s:", names[t]);
        for (int l = 0; l < 20; ++l) printf(" %d", h[t * 64 + l]);
        printf(" ... l32=%d l48=%d l63=%d\n", h[t * 64 + 32], h[t * 64 + 48], h[t * 64 + 63]);
    }
    return 0;
}
