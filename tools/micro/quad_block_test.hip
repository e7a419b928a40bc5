// Developer experiment (no GPU needed: hipcc -S and count): the world-inertia + body-force block of the Ant forward kernel
// (dsim_core.hpp: the kinematics phase behind the hand-over) in its one-link-per-lane form (k_scalar: dsim_math.hpp structs) and
// in the two backends of dsim_math_quad.hpp -- k_quad: four lanes per link, one component each, quad_perm DPP operands;
// k_quad_scalar: the same source with one link per lane (what the kernels with two environments per wavefront run).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -mllvm -amdgpu-sched-strategy=max-ilp --offload-device-only -S \
//       quad_block_test.hip -o quad_block_test.s
// result in profiles/quad_block_counts.txt
#include <hip/hip_runtime.h>
#define DSIM_FN __device__ __forceinline__
#define DSIM_OPAQUE(x) asm volatile("" : "+v"(x))
#include "../../diffrl_amd/csrc/dsim_core.hpp"

struct QuadExec {   // the two cross-lane members of the device executor that the quad backend uses
    template <int P> __device__ __forceinline__ float quad_perm(float v) {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), P, 0xf, 0xf, true));
    }
    __device__ __forceinline__ float shfl(float v, int src) { return __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(v))); }
};

extern "C" __global__ void k_scalar(const float* in, float* out) {
    const int t = threadIdx.x;
    const float* p = in + 64 * t;
    q4 rc = ldq(p); v3 com = ld3(p + 4), pc = ld3(p + 7), grav = ld3(p + 10);
    float ic0 = p[13], ic1 = p[14], ic2 = p[15], ic3 = p[16], ic4 = p[17], ic5 = p[18], m = p[19];
    sv6 wa = ldsv(p + 20), wv = ldsv(p + 26);
    const v3 cm = rotate(rc, com) + pc;
    v3 rx, ry, rz;
    rotate_basis(rc, rx, ry, rz);
    const v3 b0 = rx * ic0 + ry * ic1 + rz * ic2;
    const v3 b1 = rx * ic1 + ry * ic3 + rz * ic4;
    const v3 b2 = rx * ic2 + ry * ic4 + rz * ic5;
    inertia10 I;
    I.m = m;
    I.h = cm * m;
    const float cc = dot(cm, cm);
    I.axx = b0.x * rx.x + b1.x * ry.x + b2.x * rz.x + m * (cc - cm.x * cm.x);
    I.axy = b0.x * rx.y + b1.x * ry.y + b2.x * rz.y - m * cm.x * cm.y;
    I.axz = b0.x * rx.z + b1.x * ry.z + b2.x * rz.z - m * cm.x * cm.z;
    I.ayy = b0.y * rx.y + b1.y * ry.y + b2.y * rz.y + m * (cc - cm.y * cm.y);
    I.ayz = b0.y * rx.z + b1.y * ry.z + b2.y * rz.z - m * cm.y * cm.z;
    I.azz = b0.z * rx.z + b1.z * ry.z + b2.z * rz.z + m * (cc - cm.z * cm.z);
    const sv6 fb = inertia_mul(I, wa) + scross_dual(wv, inertia_mul(I, wv));
    const v3 mg = grav * m;
    const sv6 fg = mksv(cross(cm, mg), mg);
    float* o = out + 32 * t;
    st_i10(o, I);
    stsv(o + 10, fb - fg);
}

// the same block over a backend of dsim_math_quad.hpp; p: the link's inputs, o: its outputs (same words as k_scalar)
template <class B> __device__ __forceinline__ void quad_block(const B& b, const float* p, float* o) {
    typedef typename B::T T;
    const T rc = b.template ld<4>(p), com = b.template ld<3>(p + 4), pc = b.template ld<3>(p + 7), grav = b.template ld<3>(p + 10);
    const float ic0 = p[13], ic1 = p[14], ic2 = p[15], ic3 = p[16], ic4 = p[17], ic5 = p[18], m = p[19];
    DsimQuadSv<B> wa, wv;
    wa.w = b.template ld<3>(p + 20); wa.v = b.template ld<3>(p + 23);
    wv.w = b.template ld<3>(p + 26); wv.v = b.template ld<3>(p + 29);
    const DsimQuadBody<B> r = dq_body_inertia_force(b, rc, pc, com, grav, m, ic0, ic1, ic2, ic3, ic4, ic5, wa, wv);
    if (b.xyz()) {
        b.template st<3>(o + 4, r.I.r0);
        b.template st_from<1, 3>(o + 6, r.I.r1);
        b.template st_from<2, 3>(o + 7, r.I.r2);
        b.template st<3>(o + 1, r.I.h);
        o[0] = m;
        b.template st<3>(o + 10, r.f.w);
        b.template st<3>(o + 13, r.f.v);
    }
}
extern "C" __global__ void k_quad(const float* in, float* out) {
    const int t = threadIdx.x;
    QuadExec ex;
    DsimQuadConsts k;
    dsim_quad_consts_init(k, t);   // (the kernels keep these in registers for the whole launch: not part of the block)
    const DsimQuadLanes<QuadExec> b(ex, t, k);
    quad_block(b, in + 64 * (t >> 2), out + 32 * (t >> 2));
}
extern "C" __global__ void k_quad_scalar(const float* in, float* out) {
    const int t = threadIdx.x;
    const DsimQuadScalar b;
    quad_block(b, in + 64 * t, out + 32 * t);
}
