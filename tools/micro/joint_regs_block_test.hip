// Developer experiment (no GPU needed: hipcc -S and count): the dof-lane block of the two joint-space phases of the Ant step
// kernels, per substep, inside a substep loop as in the kernels --
//   forward (dsim_fwd_dynamics_wave): loads of the dof role, tau, qdd = H^-1 tau, the stores of tau and qdd;
//   adjoint (dsim_bwd_joint_wave):    loads of the dof role, adj tau = H^-1 adj qdd, the per-dof cotangents of tau and their stores;
// each in two forms:
//   k_*_shipped  every operand reloaded from LDS behind per-lane addresses in every substep; the mat-vec as 14 v_readlane + v_fmac
//   k_*_regs     the row of H^-1 reloaded only in a refresh substep, the joint constants (and act) loaded once per launch
//                (DsimJointRegs), the mat-vec as 14 v_fmac_f32_dpp row_newbcast:j (DevExec::row_matvec)
// and k_*_bcast: the shipped loads with the new mat-vec alone (what the kernels without room for the registers could take).
// f_tot of the dof's link is read from LDS in these forms; the f_tot block with its hand-over is counted separately below
// (k_ftot_*), as shipped and with the root's hand-over by row_newbcast:0.
// Count the instructions of each kernel's substep loop in the listing (label of the loop header to its backward branch); for the
// regs forms take out the loads that only a refresh substep executes (the block behind the refresh branch).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -mllvm -amdgpu-sched-strategy=max-ilp --offload-device-only -S \
//       joint_regs_block_test.hip -o joint_regs_block_test.s
// result in profiles/joint_regs_counts.txt
#include <hip/hip_runtime.h>
#define DSIM_FN __device__ __forceinline__
#define DSIM_OPAQUE(x) asm volatile("" : "+v"(x))
#include "../../diffrl_amd/csrc/dsim_core.hpp"

namespace {
constexpr int ND = 14;
// words of the environment's LDS block that the two blocks touch (Ant: 14 dofs, 15 coordinates, 9 links)
enum { O_q = 0, O_qd = 16, O_act = 32, O_S = 48, O_hinv = 144, O_ftot = 352, O_tau = 416, O_qdd = 432,
       O_lower = 448, O_upper = 464, O_target = 480, O_lke = 496, O_tke = 512, O_tkd = 528, O_lkd = 544,
       O_aq = 560, O_aqd = 576, O_aact = 592, O_atau = 608, O_aS = 624, O_total = 720 };

struct MicroExec {
    __device__ __forceinline__ float bcast(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }
    // (DevExec::row_matvec of dsim_hip.hip for N = 14: one asm statement, the broadcast on the multiply-add's operand)
#define RB_T(j, op) "v_fmac_f32_dpp %0, %1, %" #op " row_newbcast:" #j " row_mask:0xf bank_mask:0xf\n\t"
#define RB_14 RB_T(0, 2) RB_T(1, 3) RB_T(2, 4) RB_T(3, 5) RB_T(4, 6) RB_T(5, 7) RB_T(6, 8) RB_T(7, 9) RB_T(8, 10) RB_T(9, 11) RB_T(10, 12) \
    RB_T(11, 13) RB_T(12, 14) RB_T(13, 15)
#define RB_OPS "v"(x), "v"(h[0]), "v"(h[1]), "v"(h[2]), "v"(h[3]), "v"(h[4]), "v"(h[5]), "v"(h[6]), "v"(h[7]), "v"(h[8]), "v"(h[9]), "v"(h[10]), \
    "v"(h[11]), "v"(h[12]), "v"(h[13])
    template <int N, bool DPP_NEXT> __device__ __forceinline__ float row_matvec(const float* h, float x) {
        static_assert(N == 14, "the Ant block");
        float acc = 0.f;
        if constexpr (DPP_NEXT) asm volatile("s_nop 1\n\t" RB_14 "s_nop 1" : "+v"(acc) : RB_OPS);
        else asm volatile("s_nop 1\n\t" RB_14 : "+v"(acc) : RB_OPS);
        return acc;
    }
};

__device__ __forceinline__ void fill(float* s, const float* in) {
    for (int k = threadIdx.x; k < O_total; k += 64) s[k] = in[k];
    __syncthreads();
}
__device__ __forceinline__ void drain(const float* s, float* out) {
    __syncthreads();
    for (int k = threadIdx.x; k < O_total; k += 64) out[k] = s[k];
}
// end of a substep (the kernels: other phases that rewrite q, qd, f_tot, S and, in a refresh substep, H^-1)
__device__ __forceinline__ void next_substep() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); asm volatile("" ::: "memory"); }

template <bool REGS, bool ROW> __device__ __forceinline__ void fwd_block(float* s, const int* topo, int substeps, unsigned refresh) {
    MicroExec ex;
    const int lane = threadIdx.x;
    const bool is_dof = lane < ND;
    const int d = is_dof ? lane : 0;
    int dtype = topo[lane];
    DSIM_OPAQUE(dtype);
    const int di = topo[64 + lane], dcs = topo[128 + lane];
    DsimJointRegs jr;
    if constexpr (REGS) {   // (dsim_joint_regs_begin: once per launch, in front of the substep loop)
        const int qi0 = (dtype == DSIM_JOINT_PRISMATIC || dtype == DSIM_JOINT_REVOLUTE) ? dcs : 0;
        jr.act = s[O_act + d];
        jr.lower = s[O_lower + qi0]; jr.upper = s[O_upper + qi0]; jr.target = s[O_target + qi0];
        jr.lke = s[O_lke + di]; jr.tke = s[O_tke + di]; jr.tkd = s[O_tkd + di]; jr.lkd = s[O_lkd + di];
    }
    for (int sub = 0; sub < substeps; ++sub) {
        const bool update_mass = ((refresh >> sub) & 1u) != 0;   // (the kernels: a flag of the substep loop)
        const bool hinge = dtype == DSIM_JOINT_PRISMATIC || dtype == DSIM_JOINT_REVOLUTE;
        const int qi = hinge ? dcs : 0;
        const sv6 Sd = ldsv(s + O_S + 6 * d);
        const float q_d = s[O_q + qi], qd_d = s[O_qd + d];
        float act_d, lower, upper, target, lke, tke, tkd, lkd;
        float hrow_l[ND];
        const float* hrow = hrow_l;
        if constexpr (REGS) {
            if (update_mass) {   // (the launch's first substep is a refresh substep)
#pragma unroll
                for (int j = 0; j < ND; ++j) jr.hrow[j] = s[O_hinv + d * ND + j];
            }
            act_d = jr.act; lower = jr.lower; upper = jr.upper; target = jr.target;
            lke = jr.lke; tke = jr.tke; tkd = jr.tkd; lkd = jr.lkd;
            hrow = jr.hrow;
        } else {
            act_d = s[O_act + d];
            lower = s[O_lower + qi]; upper = s[O_upper + qi]; target = s[O_target + qi];
            lke = s[O_lke + di]; tke = s[O_tke + di]; tkd = s[O_tkd + di]; lkd = s[O_lkd + di];
#pragma unroll
            for (int j = 0; j < ND; ++j) hrow_l[j] = s[O_hinv + d * ND + j];
        }
        const sv6 F = ldsv(s + O_ftot + 6 * di);
        float t = 0.0f - sdot(Sd, F);
        if (hinge) {
            float limit_f = 0.0f;
            if (q_d < lower) limit_f = lke * (lower - q_d);
            if (q_d > upper) limit_f = lke * (upper - q_d);
            t = t - tke * (q_d - target) - tkd * qd_d + act_d + limit_f - lkd * qd_d;
        }
        float acc;
        if constexpr (ROW) {
            acc = ex.row_matvec<ND, true>(hrow, t);
        } else {
            acc = 0.f;
#pragma unroll
            for (int j = 0; j < ND; ++j) acc += hrow[j] * ex.bcast(t, j);
        }
        if (is_dof) {
            s[O_tau + lane] = t;
            s[O_qdd + lane] = acc;
        }
        next_substep();
    }
}

template <bool REGS, bool ROW> __device__ __forceinline__ void adj_block(float* s, const int* topo, int substeps, unsigned refresh, float h) {
    MicroExec ex;
    const int lane = threadIdx.x;
    const bool is_dof = lane < ND;
    const int d = is_dof ? lane : 0;
    int type = topo[lane];
    DSIM_OPAQUE(type);
    const int i = topo[64 + lane], cs = topo[128 + lane];
    DsimJointRegs jr;
    for (int sub = substeps - 1; sub >= 0; --sub) {
        const bool update_mass = ((refresh >> sub) & 1u) != 0;   // (the kernels: a flag of the substep loop)
        const bool hinge = type == DSIM_JOINT_PRISMATIC || type == DSIM_JOINT_REVOLUTE;
        const int qi = hinge ? cs : 0;
        float hrow_l[ND];
        const float* hrow = hrow_l;
        float tke, tkd, lke, lkd, lower, upper;
        if constexpr (REGS) {
            if (!jr.h_ok) {
#pragma unroll
                for (int j = 0; j < ND; ++j) jr.hrow[j] = s[O_hinv + d * ND + j];
            }
            if (!jr.c_ok) {
                jr.tke = s[O_tke + i]; jr.tkd = s[O_tkd + i]; jr.lke = s[O_lke + i]; jr.lkd = s[O_lkd + i];
                jr.lower = s[O_lower + qi]; jr.upper = s[O_upper + qi];
                jr.c_ok = true;
            }
            jr.h_ok = !update_mass;
            tke = jr.tke; tkd = jr.tkd; lke = jr.lke; lkd = jr.lkd; lower = jr.lower; upper = jr.upper;
            hrow = jr.hrow;
        } else {
#pragma unroll
            for (int j = 0; j < ND; ++j) hrow_l[j] = s[O_hinv + d * ND + j];
        }
        const sv6 ft = ldsv(s + O_ftot + 6 * i);
        const float q = s[O_q + qi];
        if constexpr (!REGS) {
            tke = s[O_tke + i]; tkd = s[O_tkd + i]; lke = s[O_lke + i]; lkd = s[O_lkd + i];
            lower = s[O_lower + qi]; upper = s[O_upper + qi];
        }
        const float g_q = s[O_aq + qi], g_qd_in = s[O_aqd + d], g_act = s[O_aact + d];
        const float g = g_qd_in + h * g_q;
        const float aqdd = h * g;
        float at;
        if constexpr (ROW) {
            at = ex.row_matvec<ND, false>(hrow, aqdd);
        } else {
            at = 0.f;
#pragma unroll
            for (int j = 0; j < ND; ++j) at += hrow[j] * ex.bcast(aqdd, j);
        }
        if (is_dof) {
            s[O_atau + lane] = at;
            stsv(s + O_aS + 6 * lane, ft * (-at));
            if (hinge) {
                float dq = -tke;
                if (q < lower) dq = -tke - lke;
                if (q > upper) dq = -tke - lke;
                s[O_aq + qi] = g_q + dq * at;
                s[O_aqd + lane] = g + (-tkd - lkd) * at;
                s[O_aact + lane] = g_act + at;
            } else {
                s[O_aqd + lane] = g;
            }
        }
        next_substep();
    }
}

// ---- the forward's f_tot block as shipped (dsim_fwd_ftot_rowtree + the hand-over of dsim_fwd_dynamics_wave): one link per lane on
// six registers -- f + cwb, five row-tree steps of six v_fmac_f32_dpp (Ant: RT_N = 5; two wave shifts, row shifts by 3, 5, 7, the
// step weights per lane), the store of f_tot, then f_tot[link(d)] to the dof lanes: one row shift per component, the root's six
// by v_readlane (ROOT_BCAST: by a row_newbcast:0 move, the candidate the issue names) and a select.  tau's dot product with S_d
// keeps the result alive.  The quad form of part C is NOT here (not written: see profiles/joint_regs_counts.txt).
enum { O_f = 0, O_cwb = 64, O_ft = 128, O_S2 = 192, O_t2 = 288, O_total2 = 320 };
template <int D, bool FIRST> __device__ __forceinline__ void add_shift(float& a0, float& a1, float& a2, float& a3, float& a4, float& a5, float w) {
    if constexpr (FIRST) asm volatile("s_nop 1" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5));
    if constexpr (D == 0)
        asm volatile("v_fmac_f32_dpp %0, %0, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %1, %1, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %2, %2, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %3, %3, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %4, %4, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %5, %5, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5) : "v"(w));
    else
        asm volatile("v_fmac_f32_dpp %0, %0, %6 row_shl:%7 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %1, %1, %6 row_shl:%7 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %2, %2, %6 row_shl:%7 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %3, %3, %6 row_shl:%7 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %4, %4, %6 row_shl:%7 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %5, %5, %6 row_shl:%7 row_mask:0xf bank_mask:0xf bound_ctrl:1"
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5) : "v"(w), "n"(D));
}
template <int CTRL> __device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
template <bool ROOT_BCAST> __device__ __forceinline__ void ftot_block(float* s, const float* wts, int substeps) {
    MicroExec ex;
    const int lane = threadIdx.x;
    const bool is_link = lane < 9, is_dof = lane < ND;
    const int l = is_link ? lane : 0, d = is_dof ? lane : 0;
    const float w1 = wts[lane], w2 = wts[64 + lane], w3 = wts[128 + lane], w4 = wts[192 + lane], w5 = wts[256 + lane];
    for (int sub = 0; sub < substeps; ++sub) {
        const sv6 f = ldsv(s + O_f + 6 * l), cw = ldsv(s + O_cwb + 6 * l), Sd = ldsv(s + O_S2 + 6 * d);
        float a0 = f.w.x + cw.w.x, a1 = f.w.y + cw.w.y, a2 = f.w.z + cw.w.z, a3 = f.v.x + cw.v.x, a4 = f.v.y + cw.v.y, a5 = f.v.z + cw.v.z;
        add_shift<0, true>(a0, a1, a2, a3, a4, a5, w1);
        add_shift<0, false>(a0, a1, a2, a3, a4, a5, w2);
        add_shift<3, false>(a0, a1, a2, a3, a4, a5, w3);
        add_shift<5, false>(a0, a1, a2, a3, a4, a5, w4);
        add_shift<7, false>(a0, a1, a2, a3, a4, a5, w5);
        if (is_link) stsv(s + O_ft + 6 * lane, mksv(mk3(a0, a1, a2), mk3(a3, a4, a5)));
        // hand-over: dof lane d holds link d - 5's total (row_shr:5); the root's six dofs take lane 0's
        sv6 F = mksv(mk3(dpp_mov<0x115>(a0), dpp_mov<0x115>(a1), dpp_mov<0x115>(a2)), mk3(dpp_mov<0x115>(a3), dpp_mov<0x115>(a4), dpp_mov<0x115>(a5)));
        sv6 Fr;
        if constexpr (ROOT_BCAST)
            Fr = mksv(mk3(dpp_mov<0x150>(a0), dpp_mov<0x150>(a1), dpp_mov<0x150>(a2)), mk3(dpp_mov<0x150>(a3), dpp_mov<0x150>(a4), dpp_mov<0x150>(a5)));
        else
            Fr = mksv(mk3(ex.bcast(a0, 0), ex.bcast(a1, 0), ex.bcast(a2, 0)), mk3(ex.bcast(a3, 0), ex.bcast(a4, 0), ex.bcast(a5, 0)));
        if (lane < 6) F = Fr;
        const float t = 0.0f - sdot(Sd, F);
        if (is_dof) s[O_t2 + lane] = t;
        next_substep();
    }
}
}  // namespace

// `off` (0 at run time) keeps the compiler from proving more than word alignment of the block's arrays: in the kernels they sit
// behind per-environment offsets and every load below is a single-word load, as counted in profiles/joint_regs_counts.txt
#define DSIM_MICRO_KERNEL(name, call)                                                                                      \
    extern "C" __global__ void name(const float* in, const int* topo, float* out, int substeps, unsigned refresh, float h, int off) { \
        __shared__ float s0[O_total + 64];                                                                                 \
        fill(s0, in);                                                                                                      \
        float* s = s0 + off;                                                                                               \
        call;                                                                                                              \
        drain(s0, out);                                                                                                    \
    }
DSIM_MICRO_KERNEL(k_fwd_shipped, (fwd_block<false, false>(s, topo, substeps, refresh)))
DSIM_MICRO_KERNEL(k_fwd_bcast, (fwd_block<false, true>(s, topo, substeps, refresh)))
DSIM_MICRO_KERNEL(k_fwd_regs, (fwd_block<true, true>(s, topo, substeps, refresh)))
DSIM_MICRO_KERNEL(k_adj_shipped, (adj_block<false, false>(s, topo, substeps, refresh, h)))
DSIM_MICRO_KERNEL(k_adj_bcast, (adj_block<false, true>(s, topo, substeps, refresh, h)))
DSIM_MICRO_KERNEL(k_adj_regs, (adj_block<true, true>(s, topo, substeps, refresh, h)))
#define DSIM_MICRO_KERNEL2(name, call)                                                                          \
    extern "C" __global__ void name(const float* in, const float* wts, float* out, int substeps, int off) {     \
        __shared__ float s0[O_total2 + 64];                                                                     \
        for (int k = threadIdx.x; k < O_total2; k += 64) s0[k] = in[k];                                         \
        __syncthreads();                                                                                        \
        float* s = s0 + off;                                                                                    \
        call;                                                                                                   \
        __syncthreads();                                                                                        \
        for (int k = threadIdx.x; k < O_total2; k += 64) out[k] = s0[k];                                        \
    }
DSIM_MICRO_KERNEL2(k_ftot_shipped, (ftot_block<false>(s, wts, substeps)))
DSIM_MICRO_KERNEL2(k_ftot_rootbcast, (ftot_block<true>(s, wts, substeps)))
