// Developer experiment (no GPU needed: hipcc -S and count): the free root's share of the two joint-space phases of the Ant step
// kernels -- the semi-implicit Euler update of dsim_fwd_dynamics_wave (with the il word of DsimSavedIl) and integrate^T of
// dsim_bwd_joint_wave (il read in, not recomputed) -- with the data movement that belongs to them: qdd of the root's six dofs
// from the dof lanes, the stores; the six new adj qd values back to the dof lanes.  Each block in three forms:
//   k_*_shipped  one joint per lane: lane 0 alone, dsim_math.hpp structs, v_readlane to and from the dof lanes (the kernels before)
//   k_*_scalar   one joint per lane: lane 0 alone, the scalar backend of dsim_math_quad.hpp (the kernels with two environments per wave)
//   k_*_quad     one component per lane on quad 0, the quad backend of the same source, one row shift to and from the dof lanes
// k_frame is what all of them share (LDS fill, copy-out): subtract it.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -mllvm -amdgpu-sched-strategy=max-ilp --offload-device-only -S \
//       quad_joint_block_test.hip -o quad_joint_block_test.s
// result in profiles/quad_joint_counts.txt
#include <hip/hip_runtime.h>
#define DSIM_FN __device__ __forceinline__
#define DSIM_OPAQUE(x) asm volatile("" : "+v"(x))
#include "../../diffrl_amd/csrc/dsim_core.hpp"

namespace {
// words of the environment's LDS block that the two blocks touch (Ant: 14 dofs, 15 coordinates)
enum { O_q = 0, O_qd = 16, O_qdd = 32, O_aq = 48, O_aqd = 64, O_qil = 80, O_total = 96 };

struct QuadExec {
    template <int P> __device__ __forceinline__ float quad_perm(float v) {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), P, 0xf, 0xf, true));
    }
    __device__ __forceinline__ float shfl(float v, int src) { return __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(v))); }
    __device__ __forceinline__ float bcast(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }
    template <int D> __device__ __forceinline__ float from_above(float v) {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x100 + D, 0xf, 0xf, true));
    }
    template <int D> __device__ __forceinline__ float from_below(float v) {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x110 + D, 0xf, 0xf, true));
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
// the hand-over in front of the integrator's stores (Exec::mid() of a kernel without helper: a fence of the wave)
__device__ __forceinline__ void mid() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); }
}  // namespace

extern "C" __global__ void k_frame(const float* in, const int* topo, float* out, float h) {
    __shared__ float s[O_total];
    fill(s, in);
    drain(s, out);
}

// ---- forward: the integrator ------------------------------------------------------------------------------------------------------
// as shipped: the root's lane loads its 7 + 6 words, fetches qdd of its six dofs by v_readlane, integrates under its own exec
// mask and stores behind the hand-over
extern "C" __global__ void k_fwd_shipped(const float* in, const int* topo, float* out, float h) {
    __shared__ float s[O_total];
    fill(s, in);
    QuadExec ex;
    const int lane = threadIdx.x;
    int ltype = topo[lane];
    DSIM_OPAQUE(ltype);
    float qv[7], qdv[6], av[6];
#pragma unroll
    for (int k = 0; k < 7; ++k) qv[k] = s[O_q + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) qdv[k] = s[O_qd + k];
    const float acc = s[O_qdd + (lane < 14 ? lane : 0)];   // (stands for qdd = H^-1 tau of dof `lane`)
#pragma unroll
    for (int k = 0; k < 6; ++k) av[k] = ex.bcast(acc, k);
    v3 w = zero3(), pn = zero3(), vn = zero3();
    q4 rn = mkq(0.f, 0.f, 0.f, 1.f);
    const bool fr = ltype == DSIM_JOINT_FREE;
    if (fr) {
        w = mk3(qdv[0], qdv[1], qdv[2]) + mk3(av[0], av[1], av[2]) * h;
        vn = mk3(qdv[3], qdv[4], qdv[5]) + mk3(av[3], av[4], av[5]) * h;
        const v3 p = mk3(qv[0], qv[1], qv[2]);
        pn = p + (vn + cross(w, p)) * h;
        const q4 r = mkq(qv[3], qv[4], qv[5], qv[6]);
        const q4 dr = qmul_v(w, r) * 0.5f;
        const q4 rt = r + dr * h;
        const float il = dsim_inv_len(qdot(rt, rt));
        if (il > 0.0f) rn = rt * il;
        if (lane < 9) s[O_qil] = il;
    }
    mid();
    if (lane < 9 && fr) {
        st3(s + O_q, pn);
        st3(s + O_qd + 3, vn);
        stq(s + O_q + 3, rn);
        st3(s + O_qd, w);
    }
    drain(s, out);
}
extern "C" __global__ void k_fwd_scalar(const float* in, const int* topo, float* out, float h) {
    __shared__ float s[O_total];
    fill(s, in);
    QuadExec ex;
    const int lane = threadIdx.x;
    int ltype = topo[lane];
    DSIM_OPAQUE(ltype);
    float qv[7], qdv[6], av[6];
#pragma unroll
    for (int k = 0; k < 7; ++k) qv[k] = s[O_q + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) qdv[k] = s[O_qd + k];
    const float acc = s[O_qdd + (lane < 14 ? lane : 0)];
#pragma unroll
    for (int k = 0; k < 6; ++k) av[k] = ex.bcast(acc, k);
    const DsimQuadScalar b;
    DsimQuadRootStep<DsimQuadScalar> rs{};
    const bool fr = ltype == DSIM_JOINT_FREE;
    if (lane < 9 && fr) {
        rs = dq_root_integrate(b, dq4{{qv[0], qv[1], qv[2], 0.f}}, dq4{{qv[3], qv[4], qv[5], qv[6]}}, dq4{{qdv[0], qdv[1], qdv[2], 0.f}},
                               dq4{{qdv[3], qdv[4], qdv[5], 0.f}}, dq4{{av[0], av[1], av[2], 0.f}}, dq4{{av[3], av[4], av[5], 0.f}}, h);
        s[O_qil] = rs.il;
    }
    mid();
    if (lane < 9 && fr) {
        dq_st3(b, s + O_q, rs.pn);
        dq_stq(b, s + O_q + 3, rs.rn);
        dq_st3(b, s + O_qd, rs.w);
        dq_st3(b, s + O_qd + 3, rs.vn);
    }
    drain(s, out);
}
extern "C" __global__ void k_fwd_quad(const float* in, const int* topo, float* out, float h) {
    __shared__ float s[O_total];
    fill(s, in);
    QuadExec ex;
    const int lane = threadIdx.x;
    DsimQuadConsts k;
    dsim_quad_consts_init(k, lane);   // (the kernels keep the one constant used here, qs, in a register for the whole launch)
    DSIM_OPAQUE(k.qs);
    const DsimQuadLanes<QuadExec> b(ex, lane, k);
    const float rq_p = dq_ld3(b, s + O_q), rq_r = dq_ldq(b, s + O_q + 3), rq_w = dq_ld3(b, s + O_qd), rq_v = dq_ld3(b, s + O_qd + 3);
    const float acc = s[O_qdd + (lane < 14 ? lane : 0)];
    const DsimQuadRootStep<DsimQuadLanes<QuadExec>> rs = dq_root_integrate(b, rq_p, rq_r, rq_w, rq_v, acc, ex.from_above<3>(acc), h);
    if (lane == 0) s[O_qil] = rs.il;
    mid();
    if (lane < 4) {
        dq_st3(b, s + O_q, rs.pn);
        dq_stq(b, s + O_q + 3, rs.rn);
        dq_st3(b, s + O_qd, rs.w);
        dq_st3(b, s + O_qd + 3, rs.vn);
    }
    drain(s, out);
}

// ---- adjoint: integrate^T ----------------------------------------------------------------------------------------------------------
// every form ends with adj qd of dof `lane` in a register of that lane (what adj tau = H^-1 adj qdd starts from); it is stored
// here so that the compiler keeps it
extern "C" __global__ void k_adj_shipped(const float* in, const int* topo, float* out, float h) {
    __shared__ float s[O_total];
    fill(s, in);
    QuadExec ex;
    const int lane = threadIdx.x, d = lane < 14 ? lane : 0;
    int ltype = topo[lane];
    DSIM_OPAQUE(ltype);
    const float g_qd_in = s[O_aqd + d];
    float r6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (lane < 9 && ltype == DSIM_JOINT_FREE) {
        const float *qq = s + O_q, *qd = s + O_qd, *qdd = s + O_qdd;
        float* aq = s + O_aq;
        const float* aqd = s + O_aqd;
        const v3 p = ld3(qq), g_pn = ld3(aq);
        const q4 r = ldq(qq + 3), g_rn = ldq(aq + 3);
        const v3 w = ld3(qd) + ld3(qdd) * h;
        const v3 gqd_w = ld3(aqd), gqd_v = ld3(aqd + 3);
        const q4 rt = r + qmul_v(w, r) * 0.5f * h;
        q4 g_rt = mkq(0.f, 0.f, 0.f, 0.f);
        const float il = s[O_qil];
        if (il > 0.0f) {
            const q4 rn = rt * il;
            g_rt = (g_rn + rn * (-qdot(rn, g_rn))) * il;
        }
        const q4 g_r = g_rt + qmul_v(mk3(-w.x, -w.y, -w.z), g_rt) * (0.5f * h);
        const q4 g_W = qmul_adj_a(r, g_rt) * (0.5f * h);
        v3 g_w = qvec(g_W) + gqd_w;
        const v3 g_dp = g_pn * h;
        const v3 g_v = g_dp + gqd_v;
        g_w += cross(p, g_dp);
        st3(aq, g_pn - cross(w, g_dp));
        stq(aq + 3, g_r);
        r6[0] = g_w.x; r6[1] = g_w.y; r6[2] = g_w.z;
        r6[3] = g_v.x; r6[4] = g_v.y; r6[5] = g_v.z;
    }
    float g = g_qd_in;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float rk = ex.bcast(r6[k], 0);
        if (lane == k) g = rk;
    }
    if (lane < 14) s[O_aqd + lane] = g;
    drain(s, out);
}
extern "C" __global__ void k_adj_scalar(const float* in, const int* topo, float* out, float h) {
    __shared__ float s[O_total];
    fill(s, in);
    QuadExec ex;
    const int lane = threadIdx.x, d = lane < 14 ? lane : 0;
    int ltype = topo[lane];
    DSIM_OPAQUE(ltype);
    const float g_qd_in = s[O_aqd + d];
    float r6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (lane < 9 && ltype == DSIM_JOINT_FREE) {
        const DsimQuadScalar b;
        const dq4 p = dq_ld3(b, s + O_q), r = dq_ldq(b, s + O_q + 3), g_pn = dq_ld3(b, s + O_aq), g_rn = dq_ldq(b, s + O_aq + 3);
        const dq4 w = dq_axpy(b, dq_ld3(b, s + O_qdd), h, dq_ld3(b, s + O_qd));
        const dq4 rt = dq_root_rt(b, r, w, h);
        const float il = s[O_qil];
        const DsimQuadRootAdj<DsimQuadScalar> ra =
            dq_root_integrate_adj(b, p, r, w, rt, il, g_pn, g_rn, dq_ld3(b, s + O_aqd), dq_ld3(b, s + O_aqd + 3), h);
        dq_st3(b, s + O_aq, ra.aq_p);
        dq_stq(b, s + O_aq + 3, ra.aq_r);
        r6[0] = ra.g_w.c[0]; r6[1] = ra.g_w.c[1]; r6[2] = ra.g_w.c[2];
        r6[3] = ra.g_v.c[0]; r6[4] = ra.g_v.c[1]; r6[5] = ra.g_v.c[2];
    }
    float g = g_qd_in;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float rk = ex.bcast(r6[k], 0);
        if (lane == k) g = rk;
    }
    if (lane < 14) s[O_aqd + lane] = g;
    drain(s, out);
}
extern "C" __global__ void k_adj_quad(const float* in, const int* topo, float* out, float h) {
    __shared__ float s[O_total];
    fill(s, in);
    QuadExec ex;
    const int lane = threadIdx.x, d = lane < 14 ? lane : 0;
    DsimQuadConsts k;
    dsim_quad_consts_init(k, lane);
    DSIM_OPAQUE(k.qs);
    const DsimQuadLanes<QuadExec> b(ex, lane, k);
    const float g_qd_in = s[O_aqd + d];
    const float p = dq_ld3(b, s + O_q), r = dq_ldq(b, s + O_q + 3), g_pn = dq_ld3(b, s + O_aq), g_rn = dq_ldq(b, s + O_aq + 3);
    const float w = dq_axpy(b, dq_ld3(b, s + O_qdd), h, dq_ld3(b, s + O_qd));
    const float rt = dq_root_rt(b, r, w, h);
    const float il = s[O_qil];
    const DsimQuadRootAdj<DsimQuadLanes<QuadExec>> ra =
        dq_root_integrate_adj(b, p, r, w, rt, il, g_pn, g_rn, g_qd_in, ex.from_above<3>(g_qd_in), h);
    if (lane < 4) {
        dq_st3(b, s + O_aq, ra.aq_p);
        dq_stq(b, s + O_aq + 3, ra.aq_r);
    }
    float g = g_qd_in;
    const float gv = ex.from_below<3>(ra.g_v);
    if (lane < 6) g = lane < 3 ? ra.g_w : gv;
    if (lane < 14) s[O_aqd + lane] = g;
    drain(s, out);
}
