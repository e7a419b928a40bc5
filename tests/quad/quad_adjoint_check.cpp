// quad_adjoint_check.cpp -- TEST-ONLY program (tests/test_quad_adjoint_cpu.py compiles and runs it): the operations that
// diffrl_amd/csrc/dsim_math_quad.hpp adds for the adjoint's body level, on random inputs, in both backends.
//   quad backend    four lanes per value, one component each; the quads are emulated lane-serially by the host executor of
//                   tests/emu/dsim_emu.cpp, whose shfl stands in for the device's quad_perm (dsim_quad_perm)
//   scalar backend  one struct of four components per value
// Prints one line per operation:  <name> <values compared> <bit mismatches quad vs scalar> <max error vs dsim_math.hpp / scale>
// where scale is the magnitude of the operation's terms (products of the operands' norms, no further factor): both forms
// evaluate the same expression with differently ordered roundings.  Operands that the kernels read from memory (the 10 words of
// an inertia, the 10 words of its cotangent) are read from memory here too, through the backends' per-lane addresses.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#define DSIM_EMU_EXECUTOR_ONLY   // (HostExec alone: no entry points of the harness)
#include "../emu/dsim_emu.cpp"

namespace {
constexpr int NQ = 16;    // quads per wave
constexpr int NIN = 8;    // input vectors per case
constexpr int NOUT = 4;   // output vectors per case (at most)
struct Case {
    dq4 in[NIN];
    float sc[4];
    float i10[10], g10[10];
    float gout[10];   // where dq_st_g10 folds the cotangent back to its words
};
float nrm3(dq4 a) { return std::sqrt(a.c[0] * a.c[0] + a.c[1] * a.c[1] + a.c[2] * a.c[2]); }
float nrm4(dq4 a) { return std::sqrt(a.c[0] * a.c[0] + a.c[1] * a.c[1] + a.c[2] * a.c[2] + a.c[3] * a.c[3]); }
float asum(const float* p, int n) {
    float s = 0.f;
    for (int k = 0; k < n; ++k) s += std::fabs(p[k]);
    return s;
}
v3 V(dq4 a) { return mk3(a.c[0], a.c[1], a.c[2]); }
q4 Q(dq4 a) { return mkq(a.c[0], a.c[1], a.c[2], a.c[3]); }
dq4 D3(v3 a) { return dq4{{a.x, a.y, a.z, 0.f}}; }
dq4 D4(q4 a) { return dq4{{a.x, a.y, a.z, a.w}}; }
sv6 SV(const Case& k, int i) { return mksv(V(k.in[i]), V(k.in[i + 1])); }
float nsv(const Case& k, int i) { return nrm3(k.in[i]) + nrm3(k.in[i + 1]); }
template <class B> DsimQuadSv<B> QS(const typename B::T* in, int i) { return DsimQuadSv<B>{in[i], in[i + 1]}; }

// every operation: NC components of NO outputs are compared; run<B>: the header's form (k: the case's memory operands);
// ref: dsim_math.hpp's; returns the scale
struct OpLdInertiaMul {
    static constexpr const char* name = "ld_i10_mul"; static constexpr int NO = 2, NC = 3;
    template <class B> static void run(const B& b, Case& k, const typename B::T* in, typename B::T* out) {
        const DsimQuadSv<B> y = dq_inertia_mul(b, dq_ld_i10(b, k.i10), QS<B>(in, 0));
        out[0] = y.w; out[1] = y.v;
    }
    static float ref(const Case& k, dq4* o) {
        const sv6 y = inertia_mul(ld_i10(k.i10), SV(k, 0));
        o[0] = D3(y.w); o[1] = D3(y.v);
        return asum(k.i10, 10) * nsv(k, 0);
    }
};
struct OpScrossT {
    static constexpr const char* name = "scross_t"; static constexpr int NO = 2, NC = 3;
    template <class B> static void run(const B& b, Case&, const typename B::T* in, typename B::T* out) {
        const DsimQuadSv<B> y = dq_unrot(b, dq_scross_t(b, QS<B>(in, 0), QS<B>(in, 2)));
        out[0] = y.w; out[1] = y.v;
    }
    static float ref(const Case& k, dq4* o) {
        const sv6 y = scross(SV(k, 0), SV(k, 2));
        o[0] = D3(y.w); o[1] = D3(y.v);
        return nsv(k, 0) * nsv(k, 2);
    }
};
struct OpScrossDualT {   // S x* u, and acc - (a x* x + a2 x* x) through the accumulating form
    static constexpr const char* name = "scross_dual_t"; static constexpr int NO = 4, NC = 3;
    template <class B> static void run(const B& b, Case&, const typename B::T* in, typename B::T* out) {
        const DsimQuadSv<B> t = dq_scross_dual_t(b, QS<B>(in, 0), QS<B>(in, 2));
        const DsimQuadSv<B> y = dq_unrot(b, t), z = dq_unrot_sub(b, QS<B>(in, 4), dq_scross_dual_t_acc(b, t, QS<B>(in, 6), QS<B>(in, 2)));
        out[0] = y.w; out[1] = y.v; out[2] = z.w; out[3] = z.v;
    }
    static float ref(const Case& k, dq4* o) {
        const sv6 y = scross_dual(SV(k, 0), SV(k, 2)), z = SV(k, 4) - (y + scross_dual(SV(k, 6), SV(k, 2)));
        o[0] = D3(y.w); o[1] = D3(y.v); o[2] = D3(z.w); o[3] = D3(z.v);
        return (nsv(k, 0) + nsv(k, 6)) * nsv(k, 2) + nsv(k, 4);
    }
};
struct OpFcrossT {   // the cross-product pairs of f^T, added to a vector
    static constexpr const char* name = "fcross_t"; static constexpr int NO = 2, NC = 3;
    template <class B> static void run(const B& b, Case&, const typename B::T* in, typename B::T* out) {
        const DsimQuadSv<B> y = dq_unrot_add(b, QS<B>(in, 4), dq_fcross_t(b, QS<B>(in, 0), QS<B>(in, 2)));
        out[0] = y.w; out[1] = y.v;
    }
    static float ref(const Case& k, dq4* o) {
        const sv6 f = SV(k, 0), y = SV(k, 2), acc = SV(k, 4);
        o[0] = D3(acc.w + (cross(f.w, y.w) + cross(f.v, y.v)));
        o[1] = D3(acc.v + cross(f.v, y.w));
        return nsv(k, 0) * nsv(k, 2) + nsv(k, 4);
    }
};
struct OpSdot {
    static constexpr const char* name = "sdot"; static constexpr int NO = 1, NC = 3;
    template <class B> static void run(const B& b, Case&, const typename B::T* in, typename B::T* out) { out[0] = dq_sdot(b, QS<B>(in, 0), QS<B>(in, 2)); }
    static float ref(const Case& k, dq4* o) {
        const float d = sdot(SV(k, 0), SV(k, 2));
        o[0] = dq4{{d, d, d, 0.f}};
        return nsv(k, 0) * nsv(k, 2);
    }
};
struct OpQmulV {
    static constexpr const char* name = "qmul_v"; static constexpr int NO = 1, NC = 4;
    template <class B> static void run(const B& b, Case&, const typename B::T* in, typename B::T* out) { out[0] = dq_qmul_v(b, in[0], in[1]); }
    static float ref(const Case& k, dq4* o) { o[0] = D4(qmul_v(V(k.in[0]), Q(k.in[1]))); return nrm3(k.in[0]) * nrm4(k.in[1]); }
};
struct OpSvAxpy {   // S s and a s + y
    static constexpr const char* name = "sv_axpy"; static constexpr int NO = 4, NC = 3;
    template <class B> static void run(const B& b, Case& k, const typename B::T* in, typename B::T* out) {
        const DsimQuadSv<B> y = dq_sv_scale(b, QS<B>(in, 0), k.sc[0]), z = dq_sv_axpy(b, QS<B>(in, 0), k.sc[1], QS<B>(in, 2));
        out[0] = y.w; out[1] = y.v; out[2] = z.w; out[3] = z.v;
    }
    static float ref(const Case& k, dq4* o) {
        const sv6 y = SV(k, 0) * k.sc[0], z = SV(k, 2) + SV(k, 0) * k.sc[1];
        o[0] = D3(y.w); o[1] = D3(y.v); o[2] = D3(z.w); o[3] = D3(z.v);
        return nsv(k, 0) * (std::fabs(k.sc[0]) + std::fabs(k.sc[1])) + nsv(k, 2);
    }
};
// DsimQuadG back to its words 1 .. 9 (inside `if (b.xyz())`).  No kernel stores the cotangent in this form -- the body level
// reads it and turns it into a pose wrench -- so the fold lives here: it lets the rows of G + G^T be compared with the words
// that dsim_math.hpp's inertia_bilinear_adj accumulates.  Every word is written by exactly one row (its part on and above the
// diagonal), the diagonal at half its held value.
template <int R, class B> void st_sym(const B& b, float* s, typename B::T a) {
    if constexpr (B::QUAD) {
        if (R == 0 && b.c < 3) s[b.c] = a;
        if (R == 1 && (b.c == 1 || b.c == 2)) s[2 + b.c] = a;
        if (R == 2 && b.c == 2) s[5] = a;
    } else {
        if (R == 0) { s[0] = a.c[0]; s[1] = a.c[1]; s[2] = a.c[2]; }
        if (R == 1) { s[3] = a.c[1]; s[4] = a.c[2]; }
        if (R == 2) s[5] = a.c[2];
    }
}
template <class B> void dq_st_g10(const B& b, float* p, const DsimQuadG<B>& g) {
    b.template st<3>(p + 1, b.add(g.h, b.template perm<DSIM_QP_YZXW>(g.ht)));
    const typename B::T mh = b.spl(-0.5f);
    st_sym<0>(b, p + 4, b.fma(b.mul(g.r0, b.ex()), mh, g.r0));
    st_sym<1>(b, p + 4, b.fma(b.mul(g.r1, b.ey()), mh, g.r1));
    st_sym<2>(b, p + 4, b.fma(b.mul(g.r2, b.ez()), mh, g.r2));
}
// the cotangent from its words, two bilinear terms, back to the words (1 .. 9, as three vectors)
template <class B> DsimQuadG<B> two_terms(const B& b, Case& k, const typename B::T* in) {
    DsimQuadG<B> g = dq_ld_g10(b, k.g10);
    dq_inertia_bilinear_adj(b, g, QS<B>(in, 0), QS<B>(in, 2));
    dq_inertia_bilinear_adj(b, g, QS<B>(in, 4), QS<B>(in, 6));
    return g;
}
void two_terms_ref(const Case& k, float* g) {
    for (int e = 0; e < 10; ++e) g[e] = k.g10[e];
    inertia_bilinear_adj(g, SV(k, 0), SV(k, 2), 1.0f);
    inertia_bilinear_adj(g, SV(k, 4), SV(k, 6), 1.0f);
}
float two_terms_scale(const Case& k) { return asum(k.g10 + 1, 9) + nsv(k, 0) * nsv(k, 2) + nsv(k, 4) * nsv(k, 6); }
struct OpBilinearAdj {
    static constexpr const char* name = "bilinear_adj"; static constexpr int NO = 3, NC = 3;
    template <class B> static void run(const B& b, Case& k, const typename B::T* in, typename B::T* out) {
        const DsimQuadG<B> g = two_terms(b, k, in);
        if (b.xyz()) dq_st_g10(b, k.gout, g);
        out[0] = b.template ld<3>(k.gout + 1); out[1] = b.template ld<3>(k.gout + 4); out[2] = b.template ld<3>(k.gout + 7);
    }
    static constexpr bool STORES = true;   // the quad lanes read the words back only after all of them have stored
    static float ref(const Case& k, dq4* o) {
        float g[10];
        two_terms_ref(k, g);
        for (int e = 0; e < 3; ++e) o[e] = dq4{{g[1 + 3 * e], g[2 + 3 * e], g[3 + 3 * e], 0.f}};
        return two_terms_scale(k);
    }
};
struct OpPoseWrench {   // ... and that cotangent as a pose wrench, with the gravity term in[4] x in[5] joined to g_h
    static constexpr const char* name = "pose_wrench"; static constexpr int NO = 2, NC = 3;
    template <class B> static void run(const B& b, Case& k, const typename B::T* in, typename B::T* out) {
        DsimQuadG<B> g = two_terms(b, k, in);
        g.ht = dq_cross_t_acc(b, g.ht, in[4], in[5]);
        const DsimQuadWrenchT<B> W = dq_inertia_pose_wrench(b, dq_ld_i10(b, k.i10), g);
        out[0] = b.template perm<DSIM_QP_YZXW>(W.wt); out[1] = W.v;
    }
    static float ref(const Case& k, dq4* o) {
        float g[10];
        two_terms_ref(k, g);
        const inertia10 I = ld_i10(k.i10);
        sv6 W = inertia_pose_wrench(I, g);
        const v3 rg = cross(V(k.in[4]), V(k.in[5]));
        W.w += cross(I.h, rg);
        W.v += rg * I.m;
        o[0] = D3(W.w); o[1] = D3(W.v);
        return asum(k.i10, 10) * (2.f * two_terms_scale(k) + nrm3(k.in[4]) * nrm3(k.in[5]));
    }
};

template <class Op, class = void> struct Stores : std::false_type {};
template <class Op> struct Stores<Op, std::void_t<decltype(Op::STORES)>> : std::true_type {};

template <class Op> int check(int rounds, std::mt19937& rng) {
    std::normal_distribution<float> nd(0.f, 1.f);
    HostExec* ex = new HostExec;
    long n = 0, bits = 0;
    double worst = 0.0;
    for (int r = 0; r < rounds; ++r) {
        static Case cs[NQ];
        static dq4 oq[NQ][NOUT], os[NQ][NOUT], orf[NQ][NOUT];
        static float scale[NQ];
        for (int u = 0; u < NQ; ++u) {
            const float mag = std::exp(2.f * nd(rng));   // magnitudes over a few decades
            for (int i = 0; i < NIN; ++i)
                for (int e = 0; e < 4; ++e) cs[u].in[i].c[e] = nd(rng) * mag;
            for (int e = 0; e < 4; ++e) cs[u].sc[e] = nd(rng);
            for (int e = 0; e < 10; ++e) {
                cs[u].i10[e] = nd(rng);
                cs[u].g10[e] = nd(rng) * mag;
                cs[u].gout[e] = 0.f;
            }
            const DsimQuadScalar b;
            Op::run(b, cs[u], cs[u].in, os[u]);
            scale[u] = Op::ref(cs[u], orf[u]);
            for (int e = 0; e < 10; ++e) cs[u].gout[e] = 0.f;
        }
        DsimQuadConsts qc[DSIM_NL];
        ex->run([&](int lane) {
            dsim_quad_consts_init(qc[lane], lane);
            const DsimQuadLanes<HostExec> b(*ex, lane, qc[lane]);
            const int u = lane >> 2, e = lane & 3;
            float in[NIN], out[NOUT] = {};
            for (int i = 0; i < NIN; ++i) in[i] = cs[u].in[i].c[e];
            if constexpr (Stores<Op>::value) {
                // two passes: every lane of the quad stores its words in the first, the second reads them back
                Op::run(b, cs[u], in, out);
                ex->lds_fence();
            }
            Op::run(b, cs[u], in, out);
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
                    const double err = std::fabs((double)oq[u][o].c[e] - (double)orf[u][o].c[e]) / (double)scale[u];
                    if (!(err <= worst)) worst = err;   // (a NaN sticks)
                }
    }
    delete ex;
    printf("%s %ld %ld %.3e\n", Op::name, n, bits, worst);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 200;   // 16 cases each
    std::mt19937 rng(argc > 2 ? (unsigned)atoi(argv[2]) : 1234u);
    check<OpLdInertiaMul>(rounds, rng);
    check<OpScrossT>(rounds, rng);
    check<OpScrossDualT>(rounds, rng);
    check<OpFcrossT>(rounds, rng);
    check<OpSdot>(rounds, rng);
    check<OpQmulV>(rounds, rng);
    check<OpSvAxpy>(rounds, rng);
    check<OpBilinearAdj>(rounds, rng);
    check<OpPoseWrench>(rounds, rng);
    return 0;
}
