// quad_math_check.cpp -- TEST-ONLY program (tests/test_quad_math_cpu.py compiles and runs it): every operation of
// diffrl_amd/csrc/dsim_math_quad.hpp on random inputs, in both backends.
//   quad backend    four lanes per value, one component each; the quads are emulated lane-serially by the host executor of
//                   tests/emu/dsim_emu.cpp, whose shfl stands in for the device's quad_perm (dsim_quad_perm)
//   scalar backend  one struct of four components per value
// Prints one line per operation:  <name> <values compared> <bit mismatches quad vs scalar> <max error vs dsim_math.hpp / scale>
// where scale is the magnitude of the operation's terms -- the product of the operands' norms, with no further factor (unit
// quaternion: |x| for rotate, 1 for the rotation columns; sum of |Ic entries| + m (c.c + |c|) for the world inertia): both forms
// evaluate the same expression with differently ordered roundings.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#define DSIM_EMU_EXECUTOR_ONLY   // (HostExec alone: no entry points of the harness)
#include "../emu/dsim_emu.cpp"

namespace {
constexpr int NQ = 16;    // quads per wave
constexpr int NIN = 10;   // input values per case
constexpr int NOUT = 6;   // output values per case (at most)
struct Case {
    dq4 in[NIN];
    float sc[8];
};
float nrm3(dq4 a) { return std::sqrt(a.c[0] * a.c[0] + a.c[1] * a.c[1] + a.c[2] * a.c[2]); }
float nrm4(dq4 a) { return std::sqrt(a.c[0] * a.c[0] + a.c[1] * a.c[1] + a.c[2] * a.c[2] + a.c[3] * a.c[3]); }
v3 V(dq4 a) { return mk3(a.c[0], a.c[1], a.c[2]); }
q4 Q(dq4 a) { return mkq(a.c[0], a.c[1], a.c[2], a.c[3]); }
dq4 D3(v3 a) { return dq4{{a.x, a.y, a.z, 0.f}}; }
dq4 D4(q4 a) { return dq4{{a.x, a.y, a.z, a.w}}; }
inertia10 I10(const Case& k) {   // a symmetric A from in[4..6] (upper triangle), h = in[7], m = sc[0]
    inertia10 I;
    I.m = k.sc[0];
    I.h = V(k.in[7]);
    I.axx = k.in[4].c[0]; I.axy = k.in[4].c[1]; I.axz = k.in[4].c[2];
    I.ayy = k.in[5].c[1]; I.ayz = k.in[5].c[2]; I.azz = k.in[6].c[2];
    return I;
}
template <class B> DsimQuadI<B> IQ(const B& b, const typename B::T* in, const float* sc) {
    DsimQuadI<B> I;
    I.r0 = in[4]; I.r1 = in[5]; I.r2 = in[6]; I.h = in[7];
    I.m = sc[0];
    return I;
}

// every operation: NC components of NO outputs are compared; run<B>: the header's form; ref: dsim_math.hpp's; returns the scale
struct OpAdd {
    static constexpr const char* name = "add"; static constexpr int NO = 1, NC = 4;
    template <class B> static void run(const B& b, const typename B::T* in, const float*, typename B::T* out) { out[0] = b.add(in[0], in[1]); }
    static float ref(const Case& k, dq4* o) { o[0] = D4(Q(k.in[0]) + Q(k.in[1])); return nrm4(k.in[0]) + nrm4(k.in[1]); }
};
struct OpScale {
    static constexpr const char* name = "scale"; static constexpr int NO = 1, NC = 4;
    template <class B> static void run(const B& b, const typename B::T* in, const float* sc, typename B::T* out) { out[0] = dq_scale(b, in[0], sc[0]); }
    static float ref(const Case& k, dq4* o) { o[0] = D4(Q(k.in[0]) * k.sc[0]); return nrm4(k.in[0]) * std::fabs(k.sc[0]); }
};
struct OpAxpy {
    static constexpr const char* name = "axpy"; static constexpr int NO = 1, NC = 3;
    template <class B> static void run(const B& b, const typename B::T* in, const float* sc, typename B::T* out) { out[0] = dq_axpy(b, in[0], sc[0], in[1]); }
    static float ref(const Case& k, dq4* o) { o[0] = D3(V(k.in[0]) * k.sc[0] + V(k.in[1])); return nrm3(k.in[0]) * std::fabs(k.sc[0]) + nrm3(k.in[1]); }
};
struct OpCross {
    static constexpr const char* name = "cross"; static constexpr int NO = 3, NC = 3;
    template <class B> static void run(const B& b, const typename B::T* in, const float*, typename B::T* out) {
        out[0] = dq_cross(b, in[0], in[1]);
        out[1] = dq_cross_acc(b, in[2], in[0], in[1]);
        out[2] = dq_cross_sub(b, in[2], in[0], in[1]);
    }
    static float ref(const Case& k, dq4* o) {
        const v3 c = cross(V(k.in[0]), V(k.in[1]));
        o[0] = D3(c); o[1] = D3(V(k.in[2]) + c); o[2] = D3(V(k.in[2]) - c);
        return nrm3(k.in[0]) * nrm3(k.in[1]) + nrm3(k.in[2]);
    }
};
struct OpDot3 {
    static constexpr const char* name = "dot3"; static constexpr int NO = 1, NC = 3;
    template <class B> static void run(const B& b, const typename B::T* in, const float*, typename B::T* out) { out[0] = dq_dot3(b, in[0], in[1]); }
    static float ref(const Case& k, dq4* o) { const float d = dot(V(k.in[0]), V(k.in[1])); o[0] = dq4{{d, d, d, 0.f}}; return nrm3(k.in[0]) * nrm3(k.in[1]); }
};
struct OpQmul {
    static constexpr const char* name = "qmul"; static constexpr int NO = 1, NC = 4;
    template <class B> static void run(const B& b, const typename B::T* in, const float*, typename B::T* out) { out[0] = dq_qmul(b, in[0], in[1]); }
    static float ref(const Case& k, dq4* o) { o[0] = D4(qmul(Q(k.in[0]), Q(k.in[1]))); return nrm4(k.in[0]) * nrm4(k.in[1]); }
};
struct OpRotate {   // in[3]: a unit quaternion
    static constexpr const char* name = "rotate"; static constexpr int NO = 1, NC = 3;
    template <class B> static void run(const B& b, const typename B::T* in, const float*, typename B::T* out) { out[0] = dq_rotate(b, in[3], in[0]); }
    static float ref(const Case& k, dq4* o) { o[0] = D3(rotate(Q(k.in[3]), V(k.in[0]))); return nrm3(k.in[0]); }
};
struct OpRotCols {
    static constexpr const char* name = "rot_cols"; static constexpr int NO = 3, NC = 3;
    template <class B> static void run(const B& b, const typename B::T* in, const float*, typename B::T* out) {
        dq_rot_cols(b, dq_rot_pre(b, in[3]), out[0], out[1], out[2]);
    }
    static float ref(const Case& k, dq4* o) {
        v3 rx, ry, rz;
        rotate_basis(Q(k.in[3]), rx, ry, rz);
        o[0] = D3(rx); o[1] = D3(ry); o[2] = D3(rz);
        return 1.f;
    }
};
struct OpSymMul {
    static constexpr const char* name = "sym_mul"; static constexpr int NO = 1, NC = 3;
    template <class B> static void run(const B& b, const typename B::T* in, const float*, typename B::T* out) { out[0] = dq_sym_mul(b, in[4], in[5], in[6], in[0]); }
    static float ref(const Case& k, dq4* o) {
        o[0] = D3(sym_mul(I10(k), V(k.in[0])));
        return (nrm3(k.in[4]) + nrm3(k.in[5]) + nrm3(k.in[6])) * nrm3(k.in[0]);
    }
};
struct OpInertiaMul {
    static constexpr const char* name = "inertia_mul"; static constexpr int NO = 2, NC = 3;
    template <class B> static void run(const B& b, const typename B::T* in, const float* sc, typename B::T* out) {
        DsimQuadSv<B> x;
        x.w = in[0]; x.v = in[1];
        const DsimQuadSv<B> y = dq_inertia_mul(b, IQ(b, in, sc), x);
        out[0] = y.w; out[1] = y.v;
    }
    static float ref(const Case& k, dq4* o) {
        const sv6 y = inertia_mul(I10(k), mksv(V(k.in[0]), V(k.in[1])));
        o[0] = D3(y.w); o[1] = D3(y.v);
        return (nrm3(k.in[4]) + nrm3(k.in[5]) + nrm3(k.in[6]) + nrm3(k.in[7]) + std::fabs(k.sc[0])) * (nrm3(k.in[0]) + nrm3(k.in[1]));
    }
};
struct OpWorldInertia {   // in[3]: unit quaternion, in[0]: COM, sc[0]: mass, sc[1..6]: body-frame inertia
    static constexpr const char* name = "world_inertia"; static constexpr int NO = 4, NC = 3;
    template <class B> static void run(const B& b, const typename B::T* in, const float* sc, typename B::T* out) {
        typename B::T rx, ry, rz;
        dq_rot_cols(b, dq_rot_pre(b, in[3]), rx, ry, rz);
        const DsimQuadI<B> I = dq_world_inertia(b, rx, ry, rz, in[0], sc[0], sc[1], sc[2], sc[3], sc[4], sc[5], sc[6]);
        out[0] = I.r0; out[1] = I.r1; out[2] = I.r2; out[3] = I.h;
    }
    static float ref(const Case& k, dq4* o) {   // dsim_core.hpp: the one-link-per-lane form of the phase
        v3 rx, ry, rz;
        rotate_basis(Q(k.in[3]), rx, ry, rz);
        const float *s = k.sc, m = s[0];
        const v3 cm = V(k.in[0]);
        const v3 b0 = rx * s[1] + ry * s[2] + rz * s[3], b1 = rx * s[2] + ry * s[4] + rz * s[5], b2 = rx * s[3] + ry * s[5] + rz * s[6];
        const float cc = dot(cm, cm);
        const float axx = b0.x * rx.x + b1.x * ry.x + b2.x * rz.x + m * (cc - cm.x * cm.x);
        const float axy = b0.x * rx.y + b1.x * ry.y + b2.x * rz.y - m * cm.x * cm.y;
        const float axz = b0.x * rx.z + b1.x * ry.z + b2.x * rz.z - m * cm.x * cm.z;
        const float ayy = b0.y * rx.y + b1.y * ry.y + b2.y * rz.y + m * (cc - cm.y * cm.y);
        const float ayz = b0.y * rx.z + b1.y * ry.z + b2.y * rz.z - m * cm.y * cm.z;
        const float azz = b0.z * rx.z + b1.z * ry.z + b2.z * rz.z + m * (cc - cm.z * cm.z);
        o[0] = dq4{{axx, axy, axz, 0.f}}; o[1] = dq4{{axy, ayy, ayz, 0.f}}; o[2] = dq4{{axz, ayz, azz, 0.f}}; o[3] = D3(cm * m);
        float ics = 0.f;
        for (int e = 1; e <= 6; ++e) ics += std::fabs(s[e]);
        return ics + std::fabs(m) * (cc + nrm3(k.in[0]));
    }
};
struct OpScross {
    static constexpr const char* name = "scross"; static constexpr int NO = 4, NC = 3;
    template <class B> static void run(const B& b, const typename B::T* in, const float*, typename B::T* out) {
        DsimQuadSv<B> a, x, acc;
        a.w = in[0]; a.v = in[1]; x.w = in[2]; x.v = in[8]; acc.w = in[9]; acc.v = in[7];
        const DsimQuadSv<B> y = dq_scross_acc(b, acc, a, x), z = dq_scross_dual_acc(b, acc, a, x);
        out[0] = y.w; out[1] = y.v; out[2] = z.w; out[3] = z.v;
    }
    static float ref(const Case& k, dq4* o) {
        const sv6 a = mksv(V(k.in[0]), V(k.in[1])), x = mksv(V(k.in[2]), V(k.in[8])), acc = mksv(V(k.in[9]), V(k.in[7]));
        const sv6 y = acc + scross(a, x), z = acc + scross_dual(a, x);
        o[0] = D3(y.w); o[1] = D3(y.v); o[2] = D3(z.w); o[3] = D3(z.v);
        return (nrm3(k.in[0]) + nrm3(k.in[1])) * (nrm3(k.in[2]) + nrm3(k.in[8])) + nrm3(k.in[9]) + nrm3(k.in[7]);
    }
};

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
                for (int e = 0; e < 4; ++e) cs[u].in[i].c[e] = nd(rng) * (i == 3 ? 1.f : mag);
            const float qn = 1.f / nrm4(cs[u].in[3]);
            for (int e = 0; e < 4; ++e) cs[u].in[3].c[e] *= qn;
            for (int e = 0; e < 8; ++e) cs[u].sc[e] = nd(rng);
            // the rows of a symmetric matrix
            cs[u].in[5].c[0] = cs[u].in[4].c[1]; cs[u].in[6].c[0] = cs[u].in[4].c[2]; cs[u].in[6].c[1] = cs[u].in[5].c[2];
            const DsimQuadScalar b;
            Op::run(b, cs[u].in, cs[u].sc, os[u]);
            scale[u] = Op::ref(cs[u], orf[u]);
        }
        DsimQuadConsts qc[DSIM_NL];
        ex->run([&](int lane) {
            dsim_quad_consts_init(qc[lane], lane);
            const DsimQuadLanes<HostExec> b(*ex, lane, qc[lane]);
            const int u = lane >> 2, e = lane & 3;
            float in[NIN], out[NOUT] = {};
            for (int i = 0; i < NIN; ++i) in[i] = cs[u].in[i].c[e];
            Op::run(b, in, cs[u].sc, out);
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
    check<OpAdd>(rounds, rng);
    check<OpScale>(rounds, rng);
    check<OpAxpy>(rounds, rng);
    check<OpCross>(rounds, rng);
    check<OpDot3>(rounds, rng);
    check<OpQmul>(rounds, rng);
    check<OpRotate>(rounds, rng);
    check<OpRotCols>(rounds, rng);
    check<OpSymMul>(rounds, rng);
    check<OpInertiaMul>(rounds, rng);
    check<OpWorldInertia>(rounds, rng);
    check<OpScross>(rounds, rng);
    return 0;
}
