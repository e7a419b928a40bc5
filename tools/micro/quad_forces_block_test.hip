// Developer experiment (no GPU needed: hipcc -S and count): the quad kinematics block of the Ant forward kernels
// (dsim_core.hpp: dsim_fk_quad_block, four lanes per link, a tree three levels deep) per substep, inside a substep loop as in the
// kernels, in two forms:
//   k_fk_shipped  the body-level constants -- ppj[0..2], ax[1..2], com, grav, ic6[6], mass: 14 words -- reloaded from LDS behind
//                 per-lane addresses in every substep, next to the state the block reads (q, qd of the chain: 8 loads)
//   k_fk_regs     the constants loaded once, in front of the substep loop (DsimBodyRegs, dsim_body_regs_begin); the state loads stay
// Same arithmetic in both (the chain walk, dq_body_inertia_force) and the same stores, so the difference of the two loop bodies is
// what the register block removes: the loads, their address arithmetic and the waits behind them.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -mllvm -amdgpu-sched-strategy=max-ilp --offload-device-only -S \
//       quad_forces_block_test.hip -o quad_forces_block_test.s
// result in profiles/quad_forces_counts.txt
#include <hip/hip_runtime.h>
#define DSIM_FN __device__ __forceinline__
#define DSIM_OPAQUE(x) asm volatile("" : "+v"(x))
#include "../../diffrl_amd/csrc/dsim_core.hpp"

namespace {
constexpr int DEPTH = 3, L = 9;
// words of the environment's LDS block that the block touches (Ant: 9 links, 15 coordinates, 14 dofs)
enum { O_q = 0, O_qd = 16, O_xpj = 32, O_axis = 96, O_com = 128, O_grav = 160, O_ic6 = 164, O_mass = 220,
       O_xsc = 232, O_v = 296, O_a = 352, O_i10 = 408, O_f = 500, O_S = 556, O_total = 644 };

struct QuadExec {   // the cross-lane members of the device executor that the quad backend uses
    template <int P> __device__ __forceinline__ float quad_perm(float v) {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), P, 0xf, 0xf, true));
    }
    __device__ __forceinline__ float shfl(float v, int src) { return __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(v))); }
    // (k_ftot_quad: the row shifts and row folds of the device executor, dsim_hip.hip)
    template <int D> __device__ __forceinline__ float from_above(float v) {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x100 + D, 0xf, 0xf, true));
    }
    template <int D> __device__ __forceinline__ float from_below(float v) {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x110 + D, 0xf, 0xf, true));
    }
    __device__ __forceinline__ float odd_rows(float v) {
        return __int_as_float(__builtin_amdgcn_permlane16_swap(__float_as_int(v), __float_as_int(v), false, false)[1]);
    }
    __device__ __forceinline__ float upper_half(float v) {
        return __int_as_float(__builtin_amdgcn_permlane32_swap(__float_as_int(v), __float_as_int(v), false, false)[1]);
    }
};
typedef DsimQuadLanes<QuadExec> B;

// the per-lane records of the block (the kernels: DsimTopoRegs, set once per launch)
struct Topo {
    int i, on, type, ods, link[DEPTH], cs[DEPTH], ds[DEPTH];
    float w[DEPTH];
};
__device__ __forceinline__ void consts_load(const B& b, const float* s, const Topo& tp, DsimBodyRegs& br) {
    br.ppj[0] = b.template ld<3>(s + O_xpj + 7 * tp.link[0]);
#pragma unroll
    for (int p = 1; p < DEPTH; ++p) {
        br.ppj[p] = b.template ld<3>(s + O_xpj + 7 * tp.link[p]);
        br.ax[p] = b.template ld<3>(s + O_axis + 3 * tp.link[p]);
    }
    br.com = b.template ld<3>(s + O_com + 3 * tp.i);
    br.grav = b.template ld<3>(s + O_grav);
#pragma unroll
    for (int k = 0; k < 6; ++k) br.ic[k] = s[O_ic6 + 6 * tp.i + k];
    br.m = s[O_mass + tp.i];
}
// end of a substep (the kernels: the other phases, which rewrite q and qd)
__device__ __forceinline__ void next_substep() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); asm volatile("" ::: "memory"); }

template <bool REGS> __device__ __forceinline__ void fk_block(float* s, const int* topo, int substeps) {
    QuadExec ex;
    const int lane = threadIdx.x;
    DsimQuadConsts k;
    dsim_quad_consts_init(k, lane);
    DSIM_OPAQUE(k.ex); DSIM_OPAQUE(k.ey); DSIM_OPAQUE(k.ez); DSIM_OPAQUE(k.kx); DSIM_OPAQUE(k.ky); DSIM_OPAQUE(k.kz); DSIM_OPAQUE(k.qs);
    const B b(ex, lane, k);
    Topo tp;
    tp.i = topo[lane]; tp.on = topo[64 + lane]; tp.type = topo[128 + lane]; tp.ods = topo[192 + lane];
#pragma unroll
    for (int p = 0; p < DEPTH; ++p) {
        tp.link[p] = topo[256 + 64 * p + lane]; tp.cs[p] = topo[448 + 64 * p + lane]; tp.ds[p] = topo[640 + 64 * p + lane];
        tp.w[p] = (float)topo[832 + 64 * p + lane];
    }
    DsimBodyRegs br;
    if constexpr (REGS) consts_load(b, s, tp, br);   // (dsim_body_regs_begin: once per launch, in front of the substep loop)
    for (int sub = 0; sub < substeps; ++sub) {
        typedef DsimQuadSv<B> SV;
        const int i = tp.i;
        int on = tp.on, own_type = tp.type;
        DSIM_OPAQUE(on);
        DSIM_OPAQUE(own_type);
        const float *q = s + O_q, *qd = s + O_qd;
        const float qp = b.template ld<3>(q + tp.cs[0]), qr = b.template ld<4>(q + tp.cs[0] + 3);
        SV v, a, s0;
        v.w = b.template ld<3>(qd + tp.ds[0]);
        v.v = b.template ld<3>(qd + tp.ds[0] + 3);
        float ang[DEPTH], rate[DEPTH];
#pragma unroll
        for (int p = 1; p < DEPTH; ++p) {
            ang[p] = q[tp.cs[p]];
            rate[p] = qd[tp.ds[p]];
        }
        if constexpr (!REGS) consts_load(b, s, tp, br);
        float psp = b.add(qp, br.ppj[0]), rsp = qr;
        a.w = a.v = s0.w = s0.v = b.spl(0.f);
#pragma unroll
        for (int p = 1; p < DEPTH; ++p) {
            float wgt = tp.w[p];
            DSIM_OPAQUE(wgt);
            const DsimQuadRot<B> R = dq_rot_pre(b, rsp);
            const float pj = b.add(dq_rotate(b, R, dq_scale(b, br.ppj[p], wgt)), psp);
            float sn, cs;
            half_angle_sincos(ang[p] * wgt * 0.5f, sn, cs);
            const float qa = b.sel_w(dq_scale(b, br.ax[p], sn), b.spl(cs));
            const float u = dq_rotate(b, R, br.ax[p]);
            s0.w = u;
            s0.v = dq_cross(b, pj, u);
            const float r = rate[p] * wgt;
            SV vj;
            vj.w = dq_scale(b, s0.w, r);
            vj.v = dq_scale(b, s0.v, r);
            v.w = b.add(v.w, vj.w);
            v.v = b.add(v.v, vj.v);
            a = dq_scross_acc(b, a, v, vj);
            psp = pj;
            rsp = dq_qmul(b, rsp, qa);
        }
        if (on) {
            b.template st<4>(s + O_xsc + 7 * i + 3, rsp);
            if (b.xyz()) {
                b.template st<3>(s + O_xsc + 7 * i, psp);
                b.template st<3>(s + O_v + 6 * i, v.w);
                b.template st<3>(s + O_v + 6 * i + 3, v.v);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // (the kernels: Exec::mid, the hand-over to the contacts)
        const DsimQuadBody<B> body = dq_body_inertia_force(b, rsp, psp, br.com, br.grav, br.m, br.ic[0], br.ic[1], br.ic[2], br.ic[3], br.ic[4], br.ic[5], a, v);
        if (on && b.xyz()) {
            b.template st<3>(s + O_a + 6 * i, a.w);
            b.template st<3>(s + O_a + 6 * i + 3, a.v);
            float* pi = s + O_i10 + 10 * i;
            b.template st<3>(pi + 4, body.I.r0);
            b.template st_from<1, 3>(pi + 6, body.I.r1);
            b.template st_from<2, 3>(pi + 7, body.I.r2);
            b.template st<3>(pi + 1, body.I.h);
            pi[0] = br.m;
            b.template st<3>(s + O_f + 6 * i, body.f.w);
            b.template st<3>(s + O_f + 6 * i + 3, body.f.v);
            if (own_type == DSIM_JOINT_REVOLUTE) {
                float* S = s + O_S + 6 * tp.ods;
                b.template st<3>(S, s0.w);
                b.template st<3>(S + 3, s0.v);
            }
        }
        next_substep();
    }
}
// ---- NOT BUILT into the kernels, counted only: the forward's f_tot / tau block in the quad placement of the adjoint's body level
// (dsim_core.hpp: dsim_quad_tree_link -- row r of 16 lanes holds [root (row 0) | - | upper link of leg r | lower link of leg r]),
// against k_ftot_shipped of joint_regs_block_test.hip (105 issue slots: one link per lane on six registers).  f and the per-body
// contact wrench as one (w, v) pair per lane, the subtree sum by dsim_quad_tree_sum on two registers, f_tot stored by two masked
// stores, tau of a hinge = -(S . f_tot) in its link's quad (dq_sdot), handed to the hinge's dof lane by one ds_bpermute; the free
// root's S is the identity, so its six taus are -f_tot[0]: the angular three are quad 0's own lanes, the linear three come down
// by one row shift.  The sums associate as the adjoint's do, ((leg 0 + leg 1) + (leg 2 + leg 3)) + root, and the dot as two
// three-term halves: not the parent's bits.
enum { Q_f = 0, Q_cwb = 64, Q_ft = 128, Q_S = 192, Q_tau = 288, Q_total = 320 };
__device__ __forceinline__ void ftot_quad_block(float* s, const int* topo, int substeps) {
    QuadExec ex;
    const int lane = threadIdx.x;
    DsimQuadConsts k;
    dsim_quad_consts_init(k, lane);
    DSIM_OPAQUE(k.ex); DSIM_OPAQUE(k.ey); DSIM_OPAQUE(k.ez); DSIM_OPAQUE(k.qs);
    const B b(ex, lane, k);
    // per-lane records: link of the quad, whether it holds one, first dof of its hinge, and for the dof role the lane to fetch from
    const int i = topo[lane], ds = topo[128 + lane], src = topo[192 + lane];
    int on = topo[64 + lane];
    DSIM_OPAQUE(on);
    for (int sub = 0; sub < substeps; ++sub) {
        typedef DsimQuadSv<B> SV;
        const SV f = dq_ldsv(b, s + Q_f + 6 * i), cw = dq_ldsv(b, s + Q_cwb + 6 * i), S0 = dq_ldsv(b, s + Q_S + 6 * ds);
        SV x = dq_sv_add(b, f, cw);
        if (!on) {
            x.w = 0.f; x.v = 0.f;
        }
        dsim_quad_tree_sum(ex, lane, x.w);
        dsim_quad_tree_sum(ex, lane, x.v);
        if (on && b.xyz()) {
            b.template st<3>(s + Q_ft + 6 * i, x.w);
            b.template st<3>(s + Q_ft + 6 * i + 3, x.v);
        }
        const float th = dq_sdot(b, S0, x);           // every lane of the hinge's quad holds S . f_tot
        float t = ex.shfl(th, src);                   // dof lanes 6 .. 13 <- their link's quad
        if (lane < 3) t = x.w;
        const float down = ex.from_below<3>(x.v);     // dof lanes 3 .. 5 <- lanes 0 .. 2
        if (lane >= 3 && lane < 6) t = down;
        t = 0.0f - t;
        if (lane < 14) s[Q_tau + lane] = t;
        next_substep();
    }
}
}  // namespace

// `off` (0 at run time) keeps the compiler from proving more than word alignment of the block's arrays: in the kernels they sit
// behind per-environment offsets
#define DSIM_MICRO_KERNEL(name, call)                                                                  \
    extern "C" __global__ void name(const float* in, const int* topo, float* out, int substeps, int off) { \
        __shared__ float s0[O_total + 64];                                                             \
        for (int k = threadIdx.x; k < O_total; k += 64) s0[k] = in[k];                                 \
        __syncthreads();                                                                               \
        float* s = s0 + off;                                                                           \
        call;                                                                                          \
        __syncthreads();                                                                               \
        for (int k = threadIdx.x; k < O_total; k += 64) out[k] = s0[k];                                \
    }
DSIM_MICRO_KERNEL(k_fk_shipped, (fk_block<false>(s, topo, substeps)))
DSIM_MICRO_KERNEL(k_fk_regs, (fk_block<true>(s, topo, substeps)))
DSIM_MICRO_KERNEL(k_ftot_quad, (ftot_quad_block(s, topo, substeps)))
