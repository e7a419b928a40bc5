// Developer experiment (no GPU needed: hipcc -S and count): the per-link part of the Ant adjoint's body level
// (dsim_core.hpp: dsim_bwd_bodies_rowtree -- operand loads, f^T, bilinear cotangents, pose wrench, joint motion^T, scross_dual, the
// S . Wt dots, the stores) with its three subtree sums, in two forms:
//   k_scalar  one link per lane, dsim_math.hpp structs, the row-tree sums of the shipped kernels (six v_fmac_f32_dpp per step)
//   k_quad    four lanes per link over the quad backend of dsim_math_quad.hpp, subtree sums on two registers per 6-vector
// and one subtree sum alone: k_sum_scalar, k_sum_quad (row shifts + permlane swaps), k_sum_quad_bperm (row shifts + ds_bpermute).
// k_frame is what all of them share (LDS fill, copy-out): subtract it.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -mllvm -amdgpu-sched-strategy=max-ilp --offload-device-only -S \
//       quad_bwd_block_test.hip -o quad_bwd_block_test.s
// result in profiles/quad_adjoint_counts.txt
//
// Quad layout of the tree (Ant: root + four legs of two links).  Row r of 16 lanes holds four quads: [root | - | upper r | lower r]
// (the root in row 0 only).  Quads without a link carry zeros.  A subtree sum of one register is then
//   x += row_shl:4 (x)          lower -> upper            (the root reads its empty neighbour: + 0)
//   t  = x + (row 1 -> row 0, row 3 -> row 2 of x)        v_permlane16_swap
//   t += (rows 2, 3 -> rows 0, 1 of t)                    v_permlane32_swap
//   x += row_shl:8 (t)          the four uppers -> root   (the uppers and lowers read past the row's end: + 0)
// no weights.  As compiled, row_shl:4 is the DPP operand of a v_add_f32; row_shl:8 stays a v_mov_b32_dpp in front of a plain add.
#include <hip/hip_runtime.h>
#define DSIM_FN __device__ __forceinline__
#define DSIM_OPAQUE(x) asm volatile("" : "+v"(x))
#include "../../diffrl_amd/csrc/dsim_core.hpp"

namespace {
// words of the environment's LDS block that the phase touches (Ant: 9 links, 14 dofs, 15 coordinates)
enum { O_i10 = 0, O_v = 96, O_a = 160, O_af = 224, O_ai10m = 288, O_S = 384, O_aS = 480, O_qd = 576, O_aq = 600, O_aqd = 624,
       O_xsc = 648, O_agx = 720, O_grav = 832, O_total = 840 };

struct QuadExec {
    template <int P> __device__ __forceinline__ float quad_perm(float v) {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), P, 0xf, 0xf, true));
    }
    __device__ __forceinline__ float shfl(float v, int src) { return __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(v))); }
    template <int D> __device__ __forceinline__ float from_above(float v) {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x100 + D, 0xf, 0xf, true));
    }
    // rows 1, 3 of v in rows 0, 2 (v_permlane16_swap); rows 2, 3 in rows 0, 1 (v_permlane32_swap)
    __device__ __forceinline__ float odd_rows(float v) {
        return __int_as_float(__builtin_amdgcn_permlane16_swap(__float_as_int(v), __float_as_int(v), false, false)[1]);
    }
    __device__ __forceinline__ float upper_half(float v) {
        return __int_as_float(__builtin_amdgcn_permlane32_swap(__float_as_int(v), __float_as_int(v), false, false)[1]);
    }
};

__device__ __forceinline__ void fill(float* s, const float* in) {
    for (int k = threadIdx.x; k < O_total; k += 64) s[k] = in[k];
    __syncthreads();
}
__device__ __forceinline__ void drain(const float* s, float* out) {
    __syncthreads();
    if (threadIdx.x < 48) out[threadIdx.x] = s[O_aq + threadIdx.x];
}

// ---- the shipped row-tree sum of Ant (DsimDimsAnt: rt_kind = WAVE1, WAVE1, ROW, ROW, ROW; rt_d = 1, 1, 3, 5, 7) ----------------
template <bool FIRST> __device__ __forceinline__ void add_from_next(sv6& x, float w) {
    if constexpr (FIRST) asm volatile("s_nop 1" : "+v"(x.w.x), "+v"(x.w.y), "+v"(x.w.z), "+v"(x.v.x), "+v"(x.v.y), "+v"(x.v.z));
    asm volatile("v_fmac_f32_dpp %0, %0, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                 "v_fmac_f32_dpp %1, %1, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                 "v_fmac_f32_dpp %2, %2, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                 "v_fmac_f32_dpp %3, %3, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                 "v_fmac_f32_dpp %4, %4, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                 "v_fmac_f32_dpp %5, %5, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
                 : "+v"(x.w.x), "+v"(x.w.y), "+v"(x.w.z), "+v"(x.v.x), "+v"(x.v.y), "+v"(x.v.z)
                 : "v"(w));
}
template <int D> __device__ __forceinline__ void add_from_above(sv6& x, float w) {
    asm volatile("v_fmac_f32_dpp %0, %0, %6 row_shl:%7 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                 "v_fmac_f32_dpp %1, %1, %6 row_shl:%7 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                 "v_fmac_f32_dpp %2, %2, %6 row_shl:%7 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                 "v_fmac_f32_dpp %3, %3, %6 row_shl:%7 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                 "v_fmac_f32_dpp %4, %4, %6 row_shl:%7 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                 "v_fmac_f32_dpp %5, %5, %6 row_shl:%7 row_mask:0xf bank_mask:0xf bound_ctrl:1"
                 : "+v"(x.w.x), "+v"(x.w.y), "+v"(x.w.z), "+v"(x.v.x), "+v"(x.v.y), "+v"(x.v.z)
                 : "v"(w), "n"(D));
}
struct ScalarTopo {   // per-lane registers of the launch (dsim_core.hpp: DsimTopoRegs)
    int type, cs, ds;
    float w[5];
};
__device__ __forceinline__ void scalar_tree_sum(const ScalarTopo& tp, sv6& x) {
    add_from_next<true>(x, tp.w[0]);
    add_from_next<false>(x, tp.w[1]);
    add_from_above<3>(x, tp.w[2]);
    add_from_above<5>(x, tp.w[3]);
    add_from_above<7>(x, tp.w[4]);
}
__device__ __forceinline__ ScalarTopo scalar_topo(const int* topo, int lane) {
    ScalarTopo tp;
    tp.type = topo[lane]; tp.cs = topo[64 + lane]; tp.ds = topo[128 + lane];
    for (int k = 0; k < 5; ++k) {
        tp.w[k] = __int_as_float(topo[192 + 64 * k + lane]);
        DSIM_OPAQUE(tp.w[k]);
    }
    return tp;
}

// ---- the quad sums --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void quad_tree_sum(QuadExec& ex, float& x) {
#pragma clang fp contract(off)
    x = x + ex.from_above<4>(x);
    float t = x + ex.odd_rows(x);
    t = t + ex.upper_half(t);
    x = x + ex.from_above<8>(t);
}
// the leg -> root edges through the LDS crossbar instead: the root's lanes fetch the four uppers (a0 .. a3: byte addresses of
// the same component in rows 0 .. 3; the other lanes fetch a quad that holds zeros)
__device__ __forceinline__ void quad_tree_sum_bperm(QuadExec& ex, float& x, int a0, int a1, int a2, int a3) {
#pragma clang fp contract(off)
    x = x + ex.from_above<4>(x);
    const int xi = __float_as_int(x);
    const float u0 = __int_as_float(__builtin_amdgcn_ds_bpermute(a0, xi)), u1 = __int_as_float(__builtin_amdgcn_ds_bpermute(a1, xi));
    const float u2 = __int_as_float(__builtin_amdgcn_ds_bpermute(a2, xi)), u3 = __int_as_float(__builtin_amdgcn_ds_bpermute(a3, xi));
    x = x + ((u0 + u1) + (u2 + u3));
}
}  // namespace

extern "C" __global__ void k_frame(const float* in, const int* topo, float* out, int update_mass) {
    __shared__ float s[O_total];
    fill(s, in);
    drain(s, out);
}

extern "C" __global__ void k_sum_scalar(const float* in, const int* topo, float* out, int update_mass) {
    __shared__ float s[O_total];
    fill(s, in);
    const int lane = threadIdx.x;
    const ScalarTopo tp = scalar_topo(topo, lane);
    sv6 x = ldsv(s + O_v + 6 * (lane < 9 ? lane : 0));
    scalar_tree_sum(tp, x);
    if (lane < 9) stsv(s + O_aq + 6 * lane, x);   // (48 words read back)
    drain(s, out);
}
extern "C" __global__ void k_sum_quad(const float* in, const int* topo, float* out, int update_mass) {
    __shared__ float s[O_total];
    fill(s, in);
    const int lane = threadIdx.x, c = lane & 3, cl = c < 3 ? c : 2;
    QuadExec ex;
    const int li = topo[lane];
    const int i = li >= 0 ? li : 0;
    float xw = s[O_v + 6 * i + cl], xv = s[O_v + 6 * i + 3 + cl];
    quad_tree_sum(ex, xw);
    quad_tree_sum(ex, xv);
    if (li >= 0 && li < 8 && c < 3) {
        s[O_aq + 6 * i + c] = xw;
        s[O_aq + 6 * i + 3 + c] = xv;
    }
    drain(s, out);
}
extern "C" __global__ void k_sum_quad_bperm(const float* in, const int* topo, float* out, int update_mass) {
    __shared__ float s[O_total];
    fill(s, in);
    const int lane = threadIdx.x, c = lane & 3, cl = c < 3 ? c : 2;
    QuadExec ex;
    const int li = topo[lane];
    const int i = li >= 0 ? li : 0;
    int a0 = topo[64 + lane], a1 = topo[128 + lane], a2 = topo[192 + lane], a3 = topo[256 + lane];
    DSIM_OPAQUE(a0); DSIM_OPAQUE(a1); DSIM_OPAQUE(a2); DSIM_OPAQUE(a3);
    float xw = s[O_v + 6 * i + cl], xv = s[O_v + 6 * i + 3 + cl];
    quad_tree_sum_bperm(ex, xw, a0, a1, a2, a3);
    quad_tree_sum_bperm(ex, xv, a0, a1, a2, a3);
    if (li >= 0 && li < 8 && c < 3) {
        s[O_aq + 6 * i + c] = xw;
        s[O_aq + 6 * i + 3 + c] = xv;
    }
    drain(s, out);
}

// ---- the block as shipped (HAS_FREE, no ball joints, DsimFreeRootIdent; the side block's hand-over is an LDS fence here) --------
extern "C" __global__ void k_scalar(const float* in, const int* topo, float* out, int update_mass) {
    __shared__ float s[O_total];
    fill(s, in);
    const int lane = threadIdx.x;
    const ScalarTopo tp = scalar_topo(topo, lane);
    const bool on = lane < 9;
    const int i = on ? lane : 0;
    int type = tp.type;
    DSIM_OPAQUE(type);
    const int cs = tp.cs, ds = tp.ds;
    const bool hinge = type == DSIM_JOINT_PRISMATIC || type == DSIM_JOINT_REVOLUTE, fr = type == DSIM_JOINT_FREE;
    inertia10 I = ld_i10(s + O_i10 + 10 * i);
    sv6 v = ldsv(s + O_v + 6 * i), a = ldsv(s + O_a + 6 * i), r = ldsv(s + O_af + 6 * i);
    const v3 grav = ld3(s + O_grav);
    float g[10];
    for (int k = 0; k < 10; ++k) g[k] = update_mass ? s[O_ai10m + 10 * i + k] : 0.f;
    sv6 S0 = ldsv(s + O_S + 6 * ds), aS0 = ldsv(s + O_aS + 6 * ds);
    float* aq = s + O_aq;
    float* aqd = s + O_aqd;
    const float qd0 = s[O_qd + ds], g0 = aqd[ds], gq0 = aq[cs];
    const sv6 qd6 = mksv(mk3(qd0, s[O_qd + ds + 1], s[O_qd + ds + 2]), ld3(s + O_qd + ds + 3));
    const sv6 g6 = mksv(mk3(g0, aqd[ds + 1], aqd[ds + 2]), ld3(aqd + ds + 3));
    const v3 pc = ld3(s + O_xsc + 7 * i);
    const q4 rc = ldq(s + O_xsc + 7 * i + 3);
    const v3 gp = mk3(gq0, aq[cs + 1], aq[cs + 2]);
    const q4 gr = ldq(aq + cs + 3);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    const sv6 hv = inertia_mul(I, v);
    sv6 a_v, a_hv;
    a_v.w = cross(hv.w, r.w) + cross(hv.v, r.v);
    a_v.v = cross(hv.v, r.w);
    a_hv.w = cross(r.w, v.w);
    a_hv.v = cross(r.w, v.v) + cross(r.v, v.w);
    a_v += inertia_mul(I, a_hv);
    inertia_bilinear_adj(g, r, a, 1.0f);
    inertia_bilinear_adj(g, a_hv, v, 1.0f);
    sv6 W = inertia_pose_wrench(I, g);
    const v3 rg = cross(r.w, grav);
    W.w += cross(I.h, rg);
    W.v += rg * I.m;
    sv6 A = inertia_mul(I, r);
    if (!on) {
        A = zerosv();
        a_v = zerosv();
        W = zerosv();
    }
    scalar_tree_sum(tp, A);
    sv6 vj = zerosv();
    if (fr) vj = qd6;
    if (hinge) vj = S0 * qd0;
    a_v.w += cross(vj.w, A.w) + cross(vj.v, A.v);
    a_v.v += cross(vj.w, A.v);
    sv6 a_vj;
    a_vj.w = cross(A.w, v.w) + cross(A.v, v.v);
    a_vj.v = cross(A.v, v.w);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const sv6 cpose = ldsv(s + O_agx + 12 * i);
    const sv6 ctw = ldsv(s + O_agx + 12 * i + 6);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    sv6 T = a_v + ctw;
    scalar_tree_sum(tp, T);
    a_vj += T;
    sv6 Wp = zerosv();
    float aqd_new = g0;
    if (hinge) {
        Wp = scross_dual(S0, aS0 + a_vj * qd0);
        aqd_new = g0 + sdot(S0, a_vj);
    }
    sv6 Z = W + Wp + cpose;
    scalar_tree_sum(tp, Z);
    const sv6 Wt = Z - Wp;
    if (on) {
        if (hinge) {
            aqd[ds] = aqd_new;
            aq[cs] = gq0 + sdot(S0, Wt);
        }
        if (fr) {
            stsv(aqd + ds, g6 + a_vj);
            const v3 tc = Wt.w - cross(pc, Wt.v);
            st3(aq + cs, gp + Wt.v);
            stq(aq + cs + 3, gr + qmul_v(tc, rc) * 2.0f);
        }
    }
    drain(s, out);
}

// ---- four lanes per link ---------------------------------------------------------------------------------------------------------
extern "C" __global__ void k_quad(const float* in, const int* topo, float* out, int update_mass) {
    __shared__ float s[O_total];
    fill(s, in);
    const int lane = threadIdx.x;
    QuadExec ex;
    DsimQuadConsts k;
    dsim_quad_consts_init(k, lane);   // (the kernels keep these and the five words below in registers for the whole launch)
    typedef DsimQuadLanes<QuadExec> B;
    typedef DsimQuadSv<B> Sv;
    const B b(ex, lane, k);
    const int li = topo[lane], cs = topo[64 + lane], ds = topo[128 + lane];
    int type = topo[192 + lane];
    DSIM_OPAQUE(type);
    const bool on = li >= 0, fr = type == DSIM_JOINT_FREE, hinge = type == DSIM_JOINT_PRISMATIC || type == DSIM_JOINT_REVOLUTE;
    const int i = on ? li : 0, c = lane & 3;
    // ---- operands
    const DsimQuadI<B> I = dq_ld_i10(b, s + O_i10 + 10 * i);
    const Sv v = dq_ldsv(b, s + O_v + 6 * i), a = dq_ldsv(b, s + O_a + 6 * i), r = dq_ldsv(b, s + O_af + 6 * i);
    const float grav = b.ld<3>(s + O_grav);
    DsimQuadG<B> g = dq_ld_g10(b, s + O_ai10m + 10 * i);
    if (!update_mass) g = dq_g10_zero(b);
    const Sv S0 = dq_ldsv(b, s + O_S + 6 * ds), aS0 = dq_ldsv(b, s + O_aS + 6 * ds);
    float* aq = s + O_aq;
    float* aqd = s + O_aqd;
    // hinge: the dof's / coordinate's word in every lane; free root: words c and 3 + c of its six dofs / seven coordinates
    const int dl = fr ? (c < 3 ? c : 2) : 0;
    const Sv qd6{s[O_qd + ds + dl], b.ld<3>(s + O_qd + ds + 3)}, g6{aqd[ds + dl], b.ld<3>(aqd + ds + 3)};
    const float qd0 = qd6.w, g0 = g6.w, gp = aq[cs + dl];
    const float pc = b.ld<3>(s + O_xsc + 7 * i), rc = b.ld<4>(s + O_xsc + 7 * i + 3), gr = b.ld<4>(aq + cs + 3);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    // ---- f^T, bilinear cotangents, pose wrench of inertia + gravity
    const Sv hv = dq_inertia_mul(b, I, v);
    Sv av_t = dq_fcross_t(b, hv, r);
    const Sv ahv = dq_unrot(b, dq_scross_t(b, r, v));
    Sv av = dq_inertia_mul(b, I, ahv);
    dq_inertia_bilinear_adj(b, g, r, a);
    dq_inertia_bilinear_adj(b, g, ahv, v);
    g.ht = dq_cross_t_acc(b, g.ht, r.w, grav);
    DsimQuadWrenchT<B> W = dq_inertia_pose_wrench(b, I, g);
    Sv A = dq_inertia_mul(b, I, r);
    if (!on) {
        A.w = 0.f; A.v = 0.f;
        W.wt = 0.f; W.v = 0.f;
    }
    quad_tree_sum(ex, A.w);
    quad_tree_sum(ex, A.v);
    // ---- joint motion^T
    Sv vj = dq_sv_scale(b, S0, qd0);
    if (fr) vj = qd6;
    av_t = dq_scross_dual_t_acc(b, av_t, vj, A);
    const Sv avj_t = dq_fcross_t(b, A, v);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const Sv cpose = dq_ldsv(b, s + O_agx + 12 * i), ctw = dq_ldsv(b, s + O_agx + 12 * i + 6);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    Sv T = dq_sv_add(b, dq_unrot_add(b, av, av_t), ctw);
    if (!on) {
        T.w = 0.f; T.v = 0.f;
    }
    quad_tree_sum(ex, T.w);
    quad_tree_sum(ex, T.v);
    const Sv avj = dq_unrot_add(b, T, avj_t);
    // ---- hinge: S x* (aS + a_vj qd), adj qd
    Sv Wp_t = dq_scross_dual_t(b, S0, dq_sv_axpy(b, avj, qd0, aS0));
    if (!hinge) {
        Wp_t.w = 0.f; Wp_t.v = 0.f;
    }
    const float aqd_new = b.add(g0, dq_sdot(b, S0, avj));
    Sv Z;
    Z.w = b.add(cpose.w, b.perm<DSIM_QP_YZXW>(b.add(W.wt, Wp_t.w)));
    Z.v = b.add(cpose.v, b.add(W.v, b.perm<DSIM_QP_YZXW>(Wp_t.v)));
    if (!on) {
        Z.w = 0.f; Z.v = 0.f;
    }
    quad_tree_sum(ex, Z.w);
    quad_tree_sum(ex, Z.v);
    const Sv Wt = dq_unrot_sub(b, Z, Wp_t);
    // ---- adj q; the stores
    const float aq_new = b.add(gp, dq_sdot(b, S0, Wt));
    const Sv aqd6 = dq_sv_add(b, g6, avj);
    const float tc = dq_cross_sub(b, Wt.w, pc, Wt.v);
    const float aqp = b.add(gp, Wt.v), aqr = b.fma(dq_qmul_v(b, tc, rc), 2.f, gr);
    if (on && (c == 0 || (fr && c < 3))) {
        aqd[ds + c] = fr ? aqd6.w : aqd_new;
        aq[cs + c] = fr ? aqp : aq_new;
    }
    if (fr && c < 3) aqd[ds + 3 + c] = aqd6.v;
    if (fr) aq[cs + 3 + c] = aqr;
    drain(s, out);
}
