// quad_joint_check.cpp -- TEST-ONLY program (tests/test_quad_joint_cpu.py compiles and runs it): the operations that
// diffrl_amd/csrc/dsim_math_quad.hpp adds for the free root's integrator and its adjoint, and the two blocks themselves
// (dq_root_integrate, dq_root_integrate_adj), in both backends.
//   quad backend    four lanes per value, one component each; the quads are emulated lane-serially by the host executor of
//                   tests/emu/dsim_emu.cpp, whose shfl stands in for the device's quad_perm (dsim_quad_perm)
//   scalar backend  one struct of four components per value
// The reference is the scalar-struct code of dsim_math.hpp as dsim_fwd_dynamics_wave / dsim_bwd_joint_wave had it before the quad
// form (ref_integrate, ref_integrate_adj below).
// Prints one line per operation:  <name> <values compared> <bit mismatches quad vs scalar> <max error vs dsim_math.hpp / scale>
// where scale is the magnitude of the terms of the output it belongs to.  Case 0 of every round is DEGENERATE: a rotation so small
// that |r + dr h|^2 underflows (< 2^-126, here to exactly 0, which is where the host's correctly rounded 1 / sqrt gives il == 0):
// the integrator must return the identity quaternion and integrate^T a zero g_rt, in both backends, bit for bit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#define DSIM_EMU_EXECUTOR_ONLY   // (HostExec alone: no entry points of the harness)
#include "../emu/dsim_emu.cpp"

namespace {
constexpr int NQ = 16;    // quads per wave
constexpr int NIN = 10;   // input vectors per case
constexpr int NOUT = 5;   // output vectors per case (at most)
struct Case {
    dq4 in[NIN];
    float h, s;
    float mem[16];   // what the load / store operation reads and writes
    bool degenerate;
};
float nrm3(dq4 a) { return std::sqrt(a.c[0] * a.c[0] + a.c[1] * a.c[1] + a.c[2] * a.c[2]); }
float nrm4(dq4 a) { return std::sqrt(a.c[0] * a.c[0] + a.c[1] * a.c[1] + a.c[2] * a.c[2] + a.c[3] * a.c[3]); }
v3 V(dq4 a) { return mk3(a.c[0], a.c[1], a.c[2]); }
q4 Q(dq4 a) { return mkq(a.c[0], a.c[1], a.c[2], a.c[3]); }
dq4 D3(v3 a) { return dq4{{a.x, a.y, a.z, 0.f}}; }
dq4 D4(q4 a) { return dq4{{a.x, a.y, a.z, a.w}}; }
dq4 splat(float s) { return dq4{{s, s, s, s}}; }

// inputs of the two blocks: in[0] p, in[1] r (unit, or tiny in the degenerate case), in[2] qd_w, in[3] qd_v, in[4] qdd_w, in[5] qdd_v,
// in[6] g_pn, in[7] g_rn, in[8] gqd_w, in[9] gqd_v

// ---- the scalar-struct forms the kernels used (dsim_math.hpp) -----------------------------------------------------------------
struct RefStep {
    v3 pn, w, vn;
    q4 rn;
    float il;
};
RefStep ref_integrate(const Case& k) {
    const float h = k.h;
    RefStep o;
    o.w = V(k.in[2]) + V(k.in[4]) * h;
    o.vn = V(k.in[3]) + V(k.in[5]) * h;
    const v3 p = V(k.in[0]);
    o.pn = p + (o.vn + cross(o.w, p)) * h;
    const q4 r = Q(k.in[1]);
    const q4 dr = qmul_v(o.w, r) * 0.5f;
    const q4 rt = r + dr * h;
    o.il = dsim_inv_len(qdot(rt, rt));
    o.rn = mkq(0.f, 0.f, 0.f, 1.f);
    if (o.il > 0.0f) o.rn = rt * o.il;
    return o;
}
struct RefAdj {
    v3 aq_p, g_w, g_v;
    q4 aq_r;
};
RefAdj ref_integrate_adj(const Case& k, float il) {
    const float h = k.h;
    const v3 p = V(k.in[0]), g_pn = V(k.in[6]);
    const q4 r = Q(k.in[1]), g_rn = Q(k.in[7]);
    const v3 w = V(k.in[2]) + V(k.in[4]) * h;
    const v3 gqd_w = V(k.in[8]), gqd_v = V(k.in[9]);
    const q4 rt = r + qmul_v(w, r) * 0.5f * h;
    q4 g_rt = mkq(0.f, 0.f, 0.f, 0.f);
    if (il > 0.0f) {
        const q4 rn = rt * il;
        g_rt = (g_rn + rn * (-qdot(rn, g_rn))) * il;
    }
    RefAdj o;
    o.aq_r = g_rt + qmul_v(mk3(-w.x, -w.y, -w.z), g_rt) * (0.5f * h);
    const q4 g_W = qmul_adj_a(r, g_rt) * (0.5f * h);
    o.g_w = qvec(g_W) + gqd_w;
    const v3 g_dp = g_pn * h;
    o.g_v = g_dp + gqd_v;
    o.g_w += cross(p, g_dp);
    o.aq_p = g_pn - cross(w, g_dp);
    return o;
}

// every operation: NC components of NO outputs are compared; run<B>: the header's form; ref: dsim_math.hpp's, with the scale of
// every output
struct OpQdot {
    static constexpr const char* name = "qdot"; static constexpr int NO = 1, NC = 4;
    template <class B> static void run(const B& b, Case&, const typename B::T* in, typename B::T* out) { out[0] = dq_qdot(b, in[0], in[7]); }
    static void ref(const Case& k, dq4* o, float* sc) {
        o[0] = splat(qdot(Q(k.in[0]), Q(k.in[7])));
        sc[0] = nrm4(k.in[0]) * nrm4(k.in[7]);
    }
};
struct OpQmulAdjA {
    static constexpr const char* name = "qmul_adj_a"; static constexpr int NO = 1, NC = 4;
    template <class B> static void run(const B& b, Case&, const typename B::T* in, typename B::T* out) { out[0] = dq_qmul_adj_a(b, in[1], in[7]); }
    static void ref(const Case& k, dq4* o, float* sc) {
        o[0] = D4(qmul_adj_a(Q(k.in[1]), Q(k.in[7])));
        sc[0] = nrm4(k.in[1]) * nrm4(k.in[7]);
    }
};
struct OpQmulV {   // the pure-vector factor on the left, as both blocks have it
    static constexpr const char* name = "qmul_v"; static constexpr int NO = 1, NC = 4;
    template <class B> static void run(const B& b, Case&, const typename B::T* in, typename B::T* out) { out[0] = dq_qmul_v(b, in[2], in[7]); }
    static void ref(const Case& k, dq4* o, float* sc) {
        o[0] = D4(qmul_v(V(k.in[2]), Q(k.in[7])));
        sc[0] = nrm3(k.in[2]) * nrm4(k.in[7]);
    }
};
struct OpQmulVInt {   // the integrator's form: the scalar part summed in the order y, x, z
    static constexpr const char* name = "qmul_v_int"; static constexpr int NO = 1, NC = 4;
    template <class B> static void run(const B& b, Case&, const typename B::T* in, typename B::T* out) { out[0] = dq_qmul_v_int(b, in[2], in[7]); }
    static void ref(const Case& k, dq4* o, float* sc) {
        o[0] = D4(qmul_v(V(k.in[2]), Q(k.in[7])));
        sc[0] = nrm3(k.in[2]) * nrm4(k.in[7]);
    }
};
struct OpQnorm2Int {   // ... and its squared norm as one chain of four terms
    static constexpr const char* name = "qnorm2_int"; static constexpr int NO = 1, NC = 4;
    template <class B> static void run(const B& b, Case&, const typename B::T* in, typename B::T* out) { out[0] = dq_qnorm2_int(b, in[7]); }
    static void ref(const Case& k, dq4* o, float* sc) {
        o[0] = splat(qdot(Q(k.in[7]), Q(k.in[7])));
        sc[0] = nrm4(k.in[7]) * nrm4(k.in[7]);
    }
};
struct OpScaleAxpySel {   // scale, a s + y, and the select between two quaternions on a value the whole quad holds
    static constexpr const char* name = "scale_axpy_sel"; static constexpr int NO = 4, NC = 4;
    template <class B> static void run(const B& b, Case& k, const typename B::T* in, typename B::T* out) {
        out[0] = dq_scale(b, in[1], k.s);
        out[1] = dq_axpy(b, in[1], k.s, in[7]);
        const float d = b.any(dq_qdot(b, in[1], in[7]));
        out[2] = b.sel(d > 0.0f, in[1], in[7]);
        out[3] = b.sel(d > 0.0f, in[7], dq_qident(b));
    }
    static void ref(const Case& k, dq4* o, float* sc) {
        const q4 a = Q(k.in[1]), y = Q(k.in[7]);
        o[0] = D4(a * k.s);
        o[1] = D4(y + a * k.s);
        // (the select's condition through the backends' own dot product: a sum in another order could differ in sign next to 0)
        const DsimQuadScalar b;
        const bool m = b.any(dq_qdot(b, k.in[1], k.in[7])) > 0.0f;
        o[2] = m ? k.in[1] : k.in[7];
        o[3] = m ? k.in[7] : dq4{{0.f, 0.f, 0.f, 1.f}};
        sc[0] = nrm4(k.in[1]) * std::fabs(k.s);
        sc[1] = sc[0] + nrm4(k.in[7]);
        sc[2] = sc[3] = 1.f;   // (copies: exact)
    }
};
struct OpLdSt {   // a 3-vector and a quaternion through memory by per-lane address
    static constexpr const char* name = "ld_st"; static constexpr int NO = 2, NC = 4;
    template <class B> static void run(const B& b, Case& k, const typename B::T* in, typename B::T* out) {
        dq_st3(b, k.mem + 1, in[0]);
        dq_stq(b, k.mem + 5, in[1]);
        out[0] = b.sel_w(dq_ld3(b, k.mem + 1), b.spl(0.f));
        out[1] = dq_ldq(b, k.mem + 5);
    }
    static constexpr bool STORES = true;   // the quad lanes read the words back only after all of them have stored
    static void ref(const Case& k, dq4* o, float* sc) {
        o[0] = D3(V(k.in[0]));
        o[1] = k.in[1];
        sc[0] = sc[1] = 1.f;   // (copies: exact)
    }
};
struct OpRootIntegrate {
    static constexpr const char* name = "root_integrate"; static constexpr int NO = 5, NC = 4;
    template <class B> static void run(const B& b, Case& k, const typename B::T* in, typename B::T* out) {
        const DsimQuadRootStep<B> s = dq_root_integrate(b, in[0], in[1], in[2], in[3], in[4], in[5], k.h);
        const typename B::T z = b.spl(0.f);
        out[0] = b.sel_w(s.pn, z); out[1] = s.rn; out[2] = b.sel_w(s.w, z); out[3] = b.sel_w(s.vn, z); out[4] = b.spl(s.il);
    }
    static void ref(const Case& k, dq4* o, float* sc) {
        const RefStep s = ref_integrate(k);
        o[0] = D3(s.pn); o[1] = D4(s.rn); o[2] = D3(s.w); o[3] = D3(s.vn); o[4] = splat(s.il);
        sc[2] = nrm3(k.in[2]) + nrm3(k.in[4]) * k.h;
        sc[3] = nrm3(k.in[3]) + nrm3(k.in[5]) * k.h;
        sc[0] = nrm3(k.in[0]) + (sc[3] + sc[2] * nrm3(k.in[0])) * k.h;
        sc[1] = 1.f;             // a unit quaternion (or the identity)
        sc[4] = 1.f + s.il;      // 1 / |rt|
    }
};
struct OpRootIntegrateAdj {   // il as the integrator left it (DsimSavedIl), like the kernels with full checkpoints
    static constexpr const char* name = "root_integrate_adj"; static constexpr int NO = 4, NC = 4;
    template <class B> static void run(const B& b, Case& k, const typename B::T* in, typename B::T* out) {
        const typename B::T w = dq_axpy(b, in[4], k.h, in[2]);
        const typename B::T rt = dq_root_rt(b, in[1], w, k.h);
        const float il = dq_root_il(b, rt);
        const DsimQuadRootAdj<B> a = dq_root_integrate_adj(b, in[0], in[1], w, rt, il, in[6], in[7], in[8], in[9], k.h);
        const typename B::T z = b.spl(0.f);
        out[0] = b.sel_w(a.aq_p, z); out[1] = a.aq_r; out[2] = b.sel_w(a.g_w, z); out[3] = b.sel_w(a.g_v, z);
    }
    static void ref(const Case& k, dq4* o, float* sc) {
        const RefStep s = ref_integrate(k);
        const RefAdj a = ref_integrate_adj(k, s.il);
        o[0] = D3(a.aq_p); o[1] = D4(a.aq_r); o[2] = D3(a.g_w); o[3] = D3(a.g_v);
        const float w = nrm3(k.in[2]) + nrm3(k.in[4]) * k.h, gdp = nrm3(k.in[6]) * k.h;
        const float grt = k.degenerate ? 0.f : 2.f * nrm4(k.in[7]) * s.il;
        sc[0] = nrm3(k.in[6]) + w * gdp;
        sc[1] = grt * (1.f + w * 0.5f * k.h) + (k.degenerate ? 1.f : 0.f);   // (degenerate: exact zeros are expected)
        sc[2] = grt * nrm4(k.in[1]) * 0.5f * k.h + nrm3(k.in[8]) + nrm3(k.in[0]) * gdp;
        sc[3] = gdp + nrm3(k.in[9]);
    }
};

template <class Op, class = void> struct Stores : std::false_type {};
template <class Op> struct Stores<Op, std::void_t<decltype(Op::STORES)>> : std::true_type {};

long g_degenerate_bad = 0;   // degenerate cases that did not give the identity / the zero cotangent

template <class Op> void check(int rounds, std::mt19937& rng) {
    std::normal_distribution<float> nd(0.f, 1.f);
    std::uniform_real_distribution<float> ud(0.f, 1.f);
    HostExec* ex = new HostExec;
    long n = 0, bits = 0;
    double worst = 0.0;
    for (int r = 0; r < rounds; ++r) {
        static Case cs[NQ], cq[NQ];
        static dq4 oq[NQ][NOUT], os[NQ][NOUT], orf[NQ][NOUT];
        static float scale[NQ][NOUT];
        for (int u = 0; u < NQ; ++u) {
            Case& k = cs[u];
            k.degenerate = u == 0;
            const float mag = std::exp(1.5f * nd(rng));   // twists and cotangents over a few decades
            for (int i = 0; i < NIN; ++i)
                for (int e = 0; e < 4; ++e) k.in[i].c[e] = nd(rng) * (i == 0 ? 1.f : mag);
            const float rl = nrm4(k.in[1]);
            for (int e = 0; e < 4; ++e) k.in[1].c[e] *= (k.degenerate ? 1e-24f : 1.f) / rl;   // unit rotation / one whose square underflows
            k.h = std::exp(-7.f + 5.f * ud(rng));   // 1e-3 .. 0.14: |w| h from far below to beyond 1
            k.s = nd(rng);
            for (int e = 0; e < 16; ++e) k.mem[e] = 0.f;
            cq[u] = k;
            const DsimQuadScalar b;
            Op::run(b, k, k.in, os[u]);
            Op::ref(k, orf[u], scale[u]);
        }
        DsimQuadConsts qc[DSIM_NL];
        ex->run([&](int lane) {
            dsim_quad_consts_init(qc[lane], lane);
            const DsimQuadLanes<HostExec> b(*ex, lane, qc[lane]);
            const int u = lane >> 2, e = lane & 3;
            float in[NIN], out[NOUT] = {};
            for (int i = 0; i < NIN; ++i) in[i] = cq[u].in[i].c[e];
            if constexpr (Stores<Op>::value) {
                // two passes: every lane of the quad stores its words in the first, the second reads them back
                Op::run(b, cq[u], in, out);
                ex->lds_fence();
            }
            Op::run(b, cq[u], in, out);
            for (int o = 0; o < Op::NO; ++o) oq[u][o].c[e] = out[o];
        });
        for (int u = 0; u < NQ; ++u)
            for (int o = 0; o < Op::NO; ++o)
                for (int e = 0; e < Op::NC; ++e) {
                    ++n;
                    uint32_t x, y;
                    memcpy(&x, &oq[u][o].c[e], 4);
                    memcpy(&y, &os[u][o].c[e], 4);
                    if (x != y) ++bits;
                    const double err = std::fabs((double)oq[u][o].c[e] - (double)orf[u][o].c[e]) / (double)scale[u][o];
                    if (!(err <= worst)) worst = err;   // (a NaN sticks)
                }
        // the degenerate case, in both backends: identity rotation and il == 0 out of the integrator, a zero rotation cotangent
        // out of integrate^T (aq_r = g_rt + conj(W) (x) g_rt h / 2 with g_rt = 0)
        if constexpr (std::is_same<Op, OpRootIntegrate>::value) {
            for (const dq4* o : {oq[0], os[0]})
                if (!(o[1].c[0] == 0.f && o[1].c[1] == 0.f && o[1].c[2] == 0.f && o[1].c[3] == 1.f && o[4].c[0] == 0.f)) ++g_degenerate_bad;
        }
        if constexpr (std::is_same<Op, OpRootIntegrateAdj>::value) {
            for (const dq4* o : {oq[0], os[0]})
                if (!(o[1].c[0] == 0.f && o[1].c[1] == 0.f && o[1].c[2] == 0.f && o[1].c[3] == 0.f)) ++g_degenerate_bad;
        }
    }
    delete ex;
    printf("%s %ld %ld %.3e\n", Op::name, n, bits, worst);
}
}  // namespace

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 200;   // 16 cases each
    std::mt19937 rng(argc > 2 ? (unsigned)atoi(argv[2]) : 1234u);
    check<OpQdot>(rounds, rng);
    check<OpQmulAdjA>(rounds, rng);
    check<OpQmulV>(rounds, rng);
    check<OpQmulVInt>(rounds, rng);
    check<OpQnorm2Int>(rounds, rng);
    check<OpScaleAxpySel>(rounds, rng);
    check<OpLdSt>(rounds, rng);
    check<OpRootIntegrate>(rounds, rng);
    check<OpRootIntegrateAdj>(rounds, rng);
    printf("degenerate_bad %ld 0 0\n", g_degenerate_bad);
    return 0;
}
