// dsim_math_quad.hpp -- component-per-lane ("quad") forms of the 3-vector / quaternion / spatial algebra of dsim_math.hpp.
//
// A link-level phase with one link per lane uses 9 of the 64 lanes of an Ant wavefront, and every lane runs its 3-, 4- and
// 6-vector arithmetic as scalar structs.  A lone wavefront pays an issue slot per instruction whatever the instruction is, so the
// phase gets shorter only with fewer instructions: here lanes 4 i .. 4 i + 3 hold the (x, y, z, w) components of link i's
// values -- one float per lane -- and the component permutations of a cross product, a quaternion product or a matrix-vector
// product are quad_perm DPP operands (dsim_quad_perm below).
//
// Every operation is written ONCE, over a backend B:
//   DsimQuadLanes<Exec>  B::T = float, one component per lane; perm<P> is a quad_perm on the wavefront
//   DsimQuadScalar       B::T = dq4 (four floats), one link per lane; perm<P> re-orders the struct's components
// Both backends execute the same IEEE operations on every component in the same order -- the primitives are explicit
// multiplies, adds and __builtin_fmaf with contraction off -- so the two layouts give bit-identical results.  The kernels with two
// environments per wavefront (32 lanes; four lanes per link do not fit) run the scalar backend of the same phase source and
// must match the one-environment kernels bit for bit (tests/test_gpu_parity.py).
//
// A 3-vector occupies components x, y, z; what its w component holds is unspecified (finite, never read by an xyz result).
#pragma once
#include <type_traits>
#include <utility>

// Component P & 3, (P >> 2) & 3, ... of the lane's QUAD (lanes 4 k .. 4 k + 3) into its lanes 0, 1, 2, 3: the device executor
// has it as a quad_perm DPP operand (Exec::quad_perm<P>); an executor without that member (the host harness) goes through shfl.
// All four lanes of a quad must call it together.
template <class Exec, int P, class = void> struct DsimHasQuadPerm : std::false_type {};
template <class Exec, int P>
struct DsimHasQuadPerm<Exec, P, std::void_t<decltype(std::declval<Exec&>().template quad_perm<P>(0.f))>> : std::true_type {};
template <int P, class Exec> DSIM_FN float dsim_quad_perm(Exec& ex, int lane, float v) {
    if constexpr (DsimHasQuadPerm<Exec, P>::value) return ex.template quad_perm<P>(v);
    else return ex.shfl(v, (lane & ~3) | ((P >> (2 * (lane & 3))) & 3));
}

#define DSIM_QP(a, b, c, d) ((a) | ((b) << 2) | ((c) << 4) | ((d) << 6))   // quad_perm: component a -> x, b -> y, c -> z, d -> w
enum {
    DSIM_QP_XXXX = DSIM_QP(0, 0, 0, 0), DSIM_QP_YYYY = DSIM_QP(1, 1, 1, 1), DSIM_QP_ZZZZ = DSIM_QP(2, 2, 2, 2),
    DSIM_QP_WWWW = DSIM_QP(3, 3, 3, 3),
    DSIM_QP_YZXW = DSIM_QP(1, 2, 0, 3), DSIM_QP_ZXYW = DSIM_QP(2, 0, 1, 3),   // the two cyclic shifts of a cross product
    DSIM_QP_XZYW = DSIM_QP(0, 2, 1, 3), DSIM_QP_ZYXW = DSIM_QP(2, 1, 0, 3), DSIM_QP_YXZW = DSIM_QP(1, 0, 2, 3),  // q x e_k
    DSIM_QP_XYZX = DSIM_QP(0, 1, 2, 0), DSIM_QP_WWWX = DSIM_QP(3, 3, 3, 0),   // Hamilton product
    DSIM_QP_YZXY = DSIM_QP(1, 2, 0, 1), DSIM_QP_ZXYY = DSIM_QP(2, 0, 1, 1),
    DSIM_QP_ZXYZ = DSIM_QP(2, 0, 1, 2), DSIM_QP_YZXZ = DSIM_QP(1, 2, 0, 2),
    DSIM_QP_YXWZ = DSIM_QP(1, 0, 3, 2), DSIM_QP_ZWXY = DSIM_QP(2, 3, 0, 1),   // the two pair swaps of a four-term sum
    DSIM_QP_XYZY = DSIM_QP(0, 1, 2, 1), DSIM_QP_WWWY = DSIM_QP(3, 3, 3, 1),   // dq_qmul_v_int: scalar part in the order y, x, z
    DSIM_QP_YZXX = DSIM_QP(1, 2, 0, 0), DSIM_QP_ZXYX = DSIM_QP(2, 0, 1, 0)
};

// member functions (DSIM_FN is `static inline` on the host)
#if defined(__HIPCC__)
#define DSIM_MFN __device__ __forceinline__
#else
#define DSIM_MFN inline
#endif

struct dq4 {
    float c[4];
};

// ---- scalar backend: one link per lane ---------------------------------------------------------------------------------------
struct DsimQuadScalar {
    typedef dq4 T;
    static constexpr bool QUAD = false;
    template <int P> DSIM_MFN T perm(T a) const { return T{{a.c[P & 3], a.c[(P >> 2) & 3], a.c[(P >> 4) & 3], a.c[(P >> 6) & 3]}}; }
    DSIM_MFN T spl(float s) const { return T{{s, s, s, s}}; }
    DSIM_MFN T lanes(float x, float y, float z, float w) const { return T{{x, y, z, w}}; }
    DSIM_MFN T add(T a, T b) const {
#pragma clang fp contract(off)
        return T{{a.c[0] + b.c[0], a.c[1] + b.c[1], a.c[2] + b.c[2], a.c[3] + b.c[3]}};
    }
    DSIM_MFN T sub(T a, T b) const {
#pragma clang fp contract(off)
        return T{{a.c[0] - b.c[0], a.c[1] - b.c[1], a.c[2] - b.c[2], a.c[3] - b.c[3]}};
    }
    DSIM_MFN T mul(T a, T b) const {
#pragma clang fp contract(off)
        return T{{a.c[0] * b.c[0], a.c[1] * b.c[1], a.c[2] * b.c[2], a.c[3] * b.c[3]}};
    }
    DSIM_MFN T fma(T a, T b, T c) const {
        return T{{__builtin_fmaf(a.c[0], b.c[0], c.c[0]), __builtin_fmaf(a.c[1], b.c[1], c.c[1]),
                  __builtin_fmaf(a.c[2], b.c[2], c.c[2]), __builtin_fmaf(a.c[3], b.c[3], c.c[3])}};
    }
    DSIM_MFN T nfma(T a, T b, T c) const {   // c - a b
        return T{{__builtin_fmaf(-a.c[0], b.c[0], c.c[0]), __builtin_fmaf(-a.c[1], b.c[1], c.c[1]),
                  __builtin_fmaf(-a.c[2], b.c[2], c.c[2]), __builtin_fmaf(-a.c[3], b.c[3], c.c[3])}};
    }
    DSIM_MFN T sel_w(T a, T b) const { return T{{a.c[0], a.c[1], a.c[2], b.c[3]}}; }   // a's x, y, z with b's w
    // m ? a : b, m the same for all four components (a value every lane of the quad holds: dq_qdot)
    DSIM_MFN T sel(bool m, T a, T b) const { return m ? a : b; }
    // a value that is the same in all four components, as one float
    DSIM_MFN float any(T a) const { return a.c[0]; }
    // components [0, N) from p[0 .. N); the others are 0
    template <int N> DSIM_MFN T ld(const float* p) const {
        T a{{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int k = 0; k < N; ++k) a.c[k] = p[k];
        return a;
    }
    // components [0, N) to p[0 .. N).  Stores of 3-vectors belong inside `if (b.xyz())` (the quad backend's w lane holds nothing)
    template <int N> DSIM_MFN void st(float* p, T a) const {
#pragma unroll
        for (int k = 0; k < N; ++k) p[k] = a.c[k];
    }
    // components [N0, N) to p[N0 .. N)
    template <int N0, int N> DSIM_MFN void st_from(float* p, T a) const {
#pragma unroll
        for (int k = N0; k < N; ++k) p[k] = a.c[k];
    }
    // row R of a symmetric 3 x 3 matrix kept as six words s = (xx, xy, xz, yy, yz, zz): (xx, xy, xz), (xy, yy, yz), (xz, yz, zz)
    template <int R> DSIM_MFN T ld_sym(const float* s) const {
        return R == 0 ? T{{s[0], s[1], s[2], 0.f}} : R == 1 ? T{{s[1], s[3], s[4], 0.f}} : T{{s[2], s[4], s[5], 0.f}};
    }
    DSIM_MFN bool xyz() const { return true; }
    // lane constants
    DSIM_MFN T ex() const { return lanes(1.f, 0.f, 0.f, 0.f); }
    DSIM_MFN T ey() const { return lanes(0.f, 1.f, 0.f, 0.f); }
    DSIM_MFN T ez() const { return lanes(0.f, 0.f, 1.f, 0.f); }
    DSIM_MFN T kx() const { return lanes(0.f, 1.f, -1.f, 0.f); }    // (q x e_x) = perm<XZY>(q) * kx
    DSIM_MFN T ky() const { return lanes(-1.f, 0.f, 1.f, 0.f); }
    DSIM_MFN T kz() const { return lanes(1.f, -1.f, 0.f, 0.f); }
    DSIM_MFN T qs() const { return lanes(1.f, 1.f, 1.f, -1.f); }    // signs of the Hamilton product's second and third terms
};

// the lane constants of the quad backend, kept in registers for the whole launch (dsim_core.hpp: DsimTopoRegs)
struct DsimQuadConsts {
    float ex, ey, ez, kx, ky, kz, qs;
};
DSIM_FN void dsim_quad_consts_init(DsimQuadConsts& k, int lane) {
    const int c = lane & 3;
    k.ex = c == 0 ? 1.f : 0.f;
    k.ey = c == 1 ? 1.f : 0.f;
    k.ez = c == 2 ? 1.f : 0.f;
    k.kx = c == 1 ? 1.f : c == 2 ? -1.f : 0.f;
    k.ky = c == 0 ? -1.f : c == 2 ? 1.f : 0.f;
    k.kz = c == 0 ? 1.f : c == 1 ? -1.f : 0.f;
    k.qs = c == 3 ? -1.f : 1.f;
}

// ---- quad backend: one component per lane -------------------------------------------------------------------------------------
template <class Exec> struct DsimQuadLanes {
    typedef float T;
    static constexpr bool QUAD = true;
    Exec& e;
    const int lane, c;   // c: this lane's component
    const DsimQuadConsts& k;
    DSIM_MFN DsimQuadLanes(Exec& e_, int lane_, const DsimQuadConsts& k_) : e(e_), lane(lane_), c(lane_ & 3), k(k_) {}
    template <int P> DSIM_MFN T perm(T a) const { return dsim_quad_perm<P>(e, lane, a); }
    DSIM_MFN T spl(float s) const { return s; }
    DSIM_MFN T add(T a, T b) const {
#pragma clang fp contract(off)
        return a + b;
    }
    DSIM_MFN T sub(T a, T b) const {
#pragma clang fp contract(off)
        return a - b;
    }
    DSIM_MFN T mul(T a, T b) const {
#pragma clang fp contract(off)
        return a * b;
    }
    DSIM_MFN T fma(T a, T b, T cc) const { return __builtin_fmaf(a, b, cc); }
    DSIM_MFN T nfma(T a, T b, T cc) const { return __builtin_fmaf(-a, b, cc); }
    DSIM_MFN T sel_w(T a, T b) const { return c == 3 ? b : a; }
    DSIM_MFN T sel(bool m, T a, T b) const { return m ? a : b; }
    DSIM_MFN float any(T a) const { return a; }
    // lanes past the vector's last component re-read it: every address stays inside the vector
    template <int N> DSIM_MFN T ld(const float* p) const { return p[c < N ? c : N - 1]; }
    template <int N> DSIM_MFN void st(float* p, T a) const { p[c] = a; }
    template <int N0, int N> DSIM_MFN void st_from(float* p, T a) const {
        if (c >= N0) p[c] = a;
    }
    // (per-lane word of the row; the w lane re-reads the z lane's)
    template <int R> DSIM_MFN T ld_sym(const float* s) const {
        return s[R == 0 ? (c < 3 ? c : 2) : R == 1 ? (c == 0 ? 1 : c == 1 ? 3 : 4) : (c == 0 ? 2 : c == 1 ? 4 : 5)];
    }
    DSIM_MFN bool xyz() const { return c < 3; }
    DSIM_MFN T ex() const { return k.ex; }
    DSIM_MFN T ey() const { return k.ey; }
    DSIM_MFN T ez() const { return k.ez; }
    DSIM_MFN T kx() const { return k.kx; }
    DSIM_MFN T ky() const { return k.ky; }
    DSIM_MFN T kz() const { return k.kz; }
    DSIM_MFN T qs() const { return k.qs; }
};

// ---- the operations, once for both backends ------------------------------------------------------------------------------------
template <class B> struct DsimQuadSv {   // spatial vector (angular, linear)
    typename B::T w, v;
};
template <class B> struct DsimQuadI {    // spatial inertia about the origin: A as three row vectors (A is symmetric up to rounding:
    typename B::T r0, r1, r2, h;         // row i times x is used as column i), first moment h = m c
    float m;
};

// On this target a quad_perm is free only as the operand of a multiply, an add or a subtract (VOP2 with a DPP source); in front of
// an fma it is an instruction of its own.  The forms below are chosen for that: at most one permuted operand per instruction, products
// whose result would need a permutation are kept in the rotated frame (dq_cross_t, dq_rotate) and permuted once, by the add or
// multiply that consumes them.
template <class B> DSIM_FN typename B::T dq_scale(const B& b, typename B::T a, float s) { return b.mul(a, b.spl(s)); }
// a s + y
template <class B> DSIM_FN typename B::T dq_axpy(const B& b, typename B::T a, float s, typename B::T y) { return b.fma(a, b.spl(s), y); }
// t with a x b = perm<YZX>(t):  t = (c_z, c_x, c_y)
template <class B> DSIM_FN typename B::T dq_cross_t(const B& b, typename B::T a, typename B::T x) {
    return b.nfma(b.template perm<DSIM_QP_YZXW>(a), x, b.mul(a, b.template perm<DSIM_QP_YZXW>(x)));
}
// t + (a x b in the same rotated frame)
template <class B> DSIM_FN typename B::T dq_cross_t_acc(const B& b, typename B::T t, typename B::T a, typename B::T x) {
    return b.nfma(b.template perm<DSIM_QP_YZXW>(a), x, b.fma(a, b.template perm<DSIM_QP_YZXW>(x), t));
}
template <class B> DSIM_FN typename B::T dq_cross(const B& b, typename B::T a, typename B::T x) {
    return b.template perm<DSIM_QP_YZXW>(dq_cross_t(b, a, x));
}
// acc + a x b, acc - a x b
template <class B> DSIM_FN typename B::T dq_cross_acc(const B& b, typename B::T acc, typename B::T a, typename B::T x) {
    return b.add(acc, b.template perm<DSIM_QP_YZXW>(dq_cross_t(b, a, x)));
}
template <class B> DSIM_FN typename B::T dq_cross_sub(const B& b, typename B::T acc, typename B::T a, typename B::T x) {
    return b.sub(acc, b.template perm<DSIM_QP_YZXW>(dq_cross_t(b, a, x)));
}
// a . b of two 3-vectors in components x, y, z -- each component adds the three products in its own cyclic order, so the three
// values may differ in the last bit; every one of them is a correctly formed dot product
template <class B> DSIM_FN typename B::T dq_dot3(const B& b, typename B::T a, typename B::T x) {
    const typename B::T p = b.mul(a, x);
    return b.add(b.add(p, b.template perm<DSIM_QP_YZXW>(p)), b.template perm<DSIM_QP_ZXYW>(p));
}
// Hamilton product (dsim_math.hpp: qmul)
template <class B> DSIM_FN typename B::T dq_qmul(const B& b, typename B::T a, typename B::T x) {
    typename B::T r = b.mul(b.template perm<DSIM_QP_WWWW>(a), x);
    r = b.fma(b.mul(b.template perm<DSIM_QP_XYZX>(a), b.qs()), b.template perm<DSIM_QP_WWWX>(x), r);
    r = b.fma(b.mul(b.template perm<DSIM_QP_YZXY>(a), b.qs()), b.template perm<DSIM_QP_ZXYY>(x), r);
    return b.nfma(b.template perm<DSIM_QP_ZXYZ>(a), b.template perm<DSIM_QP_YZXZ>(x), r);
}
// what the rotations by one quaternion share: 2 w, 2 w^2 - 1, the two cyclic shifts of q
template <class B> struct DsimQuadRot {
    typename B::T q, qy, q2z, tw, a;
};
template <class B> DSIM_FN DsimQuadRot<B> dq_rot_pre(const B& b, typename B::T q) {
    DsimQuadRot<B> R;
    const typename B::T qw = b.template perm<DSIM_QP_WWWW>(q), qz = b.template perm<DSIM_QP_ZXYW>(q);
    R.q = q;
    R.qy = b.template perm<DSIM_QP_YZXW>(q);
    R.q2z = b.add(qz, qz);
    R.tw = b.add(qw, qw);
    R.a = b.fma(R.tw, qw, b.spl(-1.f));
    return R;
}
// rotate(q, x) = x (2 w^2 - 1) + (qv x x) 2 w + qv 2 (qv . x), evaluated in the rotated frame (z, x, y) and permuted back at the end
template <class B> DSIM_FN typename B::T dq_rotate(const B& b, const DsimQuadRot<B>& R, typename B::T x) {
    typename B::T r = b.mul(b.template perm<DSIM_QP_ZXYW>(x), R.a);
    const typename B::T t = b.nfma(R.qy, x, b.mul(R.q, b.template perm<DSIM_QP_YZXW>(x)));
    r = b.fma(t, R.tw, r);
    r = b.fma(R.q2z, dq_dot3(b, R.q, x), r);
    return b.template perm<DSIM_QP_YZXW>(r);
}
template <class B> DSIM_FN typename B::T dq_rotate(const B& b, typename B::T q, typename B::T x) { return dq_rotate(b, dq_rot_pre(b, q), x); }
// columns of the rotation matrix: rotate(q, e_x), rotate(q, e_y), rotate(q, e_z) without the terms that are exactly zero:
// col_k = e_k (2 w^2 - 1) + (q x e_k) 2 w + q 2 q_k
template <class B> DSIM_FN void dq_rot_cols(const B& b, const DsimQuadRot<B>& R, typename B::T& rx, typename B::T& ry, typename B::T& rz) {
    const typename B::T qt = b.mul(R.q, R.tw), q2 = b.add(R.q, R.q);
    rx = b.fma(R.q, b.template perm<DSIM_QP_XXXX>(q2), b.fma(b.ex(), R.a, b.mul(b.template perm<DSIM_QP_XZYW>(qt), b.kx())));
    ry = b.fma(R.q, b.template perm<DSIM_QP_YYYY>(q2), b.fma(b.ey(), R.a, b.mul(b.template perm<DSIM_QP_ZYXW>(qt), b.ky())));
    rz = b.fma(R.q, b.template perm<DSIM_QP_ZZZZ>(q2), b.fma(b.ez(), R.a, b.mul(b.template perm<DSIM_QP_YXZW>(qt), b.kz())));
}
// A x for A held as three row vectors, used as columns (A symmetric)
template <class B> DSIM_FN typename B::T dq_sym_mul(const B& b, typename B::T r0, typename B::T r1, typename B::T r2, typename B::T x) {
    typename B::T y = b.mul(b.template perm<DSIM_QP_XXXX>(x), r0);
    y = b.fma(r1, b.template perm<DSIM_QP_YYYY>(x), y);
    return b.fma(r2, b.template perm<DSIM_QP_ZZZZ>(x), y);
}
// world inertia about the origin of a body with COM cm, mass m, rotation columns (rx, ry, rz) and body-frame inertia
// (ic0 .. ic5 = xx, xy, xz, yy, yz, zz):  Theta = R Ic R^T, A = Theta + m (c.c 1 - c c^T), h = m c
template <class B>
DSIM_FN DsimQuadI<B> dq_world_inertia(const B& b, typename B::T rx, typename B::T ry, typename B::T rz, typename B::T cm, float m,
                                      float ic0, float ic1, float ic2, float ic3, float ic4, float ic5) {
    typedef typename B::T T;
    const T b0 = dq_axpy(b, rz, ic2, dq_axpy(b, ry, ic1, dq_scale(b, rx, ic0)));
    const T b1 = dq_axpy(b, rz, ic4, dq_axpy(b, ry, ic3, dq_scale(b, rx, ic1)));
    const T b2 = dq_axpy(b, rz, ic5, dq_axpy(b, ry, ic4, dq_scale(b, rx, ic2)));
    DsimQuadI<B> I;
    I.m = m;
    I.h = dq_scale(b, cm, m);
    const T mcc = dq_scale(b, dq_dot3(b, cm, cm), m);
    I.r0 = b.fma(rz, b.template perm<DSIM_QP_XXXX>(b2), b.fma(ry, b.template perm<DSIM_QP_XXXX>(b1), b.mul(b.template perm<DSIM_QP_XXXX>(b0), rx)));
    I.r1 = b.fma(rz, b.template perm<DSIM_QP_YYYY>(b2), b.fma(ry, b.template perm<DSIM_QP_YYYY>(b1), b.mul(b.template perm<DSIM_QP_YYYY>(b0), rx)));
    I.r2 = b.fma(rz, b.template perm<DSIM_QP_ZZZZ>(b2), b.fma(ry, b.template perm<DSIM_QP_ZZZZ>(b1), b.mul(b.template perm<DSIM_QP_ZZZZ>(b0), rx)));
    I.r0 = b.nfma(b.template perm<DSIM_QP_XXXX>(cm), I.h, b.fma(b.ex(), mcc, I.r0));
    I.r1 = b.nfma(b.template perm<DSIM_QP_YYYY>(cm), I.h, b.fma(b.ey(), mcc, I.r1));
    I.r2 = b.nfma(b.template perm<DSIM_QP_ZZZZ>(cm), I.h, b.fma(b.ez(), mcc, I.r2));
    return I;
}
// I x = (A x.w + h x x.v, m x.v + x.w x h)
template <class B> DSIM_FN DsimQuadSv<B> dq_inertia_mul(const B& b, const DsimQuadI<B>& I, const DsimQuadSv<B>& x) {
    DsimQuadSv<B> y;
    y.w = dq_cross_acc(b, dq_sym_mul(b, I.r0, I.r1, I.r2, x.w), I.h, x.v);
    y.v = dq_cross_sub(b, dq_scale(b, x.v, I.m), I.h, x.w);
    return y;
}
// acc + a x b for spatial motion vectors: (a.w x b.w, a.v x b.w + a.w x b.v)
template <class B> DSIM_FN DsimQuadSv<B> dq_scross_acc(const B& b, const DsimQuadSv<B>& acc, const DsimQuadSv<B>& a, const DsimQuadSv<B>& x) {
    DsimQuadSv<B> y;
    y.w = dq_cross_acc(b, acc.w, a.w, x.w);
    y.v = b.add(acc.v, b.template perm<DSIM_QP_YZXW>(dq_cross_t_acc(b, dq_cross_t(b, a.v, x.w), a.w, x.v)));
    return y;
}
// acc + a x* b for a force vector b: (a.w x b.w + a.v x b.v, a.w x b.v)
template <class B> DSIM_FN DsimQuadSv<B> dq_scross_dual_acc(const B& b, const DsimQuadSv<B>& acc, const DsimQuadSv<B>& a, const DsimQuadSv<B>& x) {
    DsimQuadSv<B> y;
    y.w = b.add(acc.w, b.template perm<DSIM_QP_YZXW>(dq_cross_t_acc(b, dq_cross_t(b, a.w, x.w), a.v, x.v)));
    y.v = dq_cross_acc(b, acc.v, a.w, x.v);
    return y;
}
// What the kinematics phase computes of a link behind its pose (rc, pc), twist v and bias acceleration a: COM, world inertia about
// the origin and the body force  f = I a + v x* (I v) - (cm x m g, m g)
template <class B> struct DsimQuadBody {
    DsimQuadI<B> I;
    DsimQuadSv<B> f;
};
template <class B>
DSIM_FN DsimQuadBody<B> dq_body_inertia_force(const B& b, typename B::T rc, typename B::T pc, typename B::T com, typename B::T grav, float m,
                                              float ic0, float ic1, float ic2, float ic3, float ic4, float ic5,
                                              const DsimQuadSv<B>& a, const DsimQuadSv<B>& v) {
    typedef typename B::T T;
    const DsimQuadRot<B> R = dq_rot_pre(b, rc);
    const T cm = b.add(dq_rotate(b, R, com), pc);
    T rx, ry, rz;
    dq_rot_cols(b, R, rx, ry, rz);
    DsimQuadBody<B> r;
    r.I = dq_world_inertia(b, rx, ry, rz, cm, m, ic0, ic1, ic2, ic3, ic4, ic5);
    const DsimQuadSv<B> fb = dq_scross_dual_acc(b, dq_inertia_mul(b, r.I, a), v, dq_inertia_mul(b, r.I, v));
    const T mg = dq_scale(b, grav, m);
    r.f.w = dq_cross_acc(b, fb.w, mg, cm);
    r.f.v = b.sub(fb.v, mg);
    return r;
}

// ---- the adjoint's body level (dsim_core.hpp: dsim_bwd_bodies_rowtree) ---------------------------------------------------------
// Sums of cross products stay in the ROTATED frame of dq_cross_t (t = (c_z, c_x, c_y)) for as long as they are only added to:
// dq_cross_t_acc chains them at two instructions each, and the one permutation back rides on the add or subtract that
// consumes the sum (dq_unrot_add / dq_unrot_sub).  A DsimQuadSv whose name ends in _t holds both halves in that frame.
template <class B> DSIM_FN DsimQuadSv<B> dq_ldsv(const B& b, const float* p) {
    DsimQuadSv<B> x;
    x.w = b.template ld<3>(p);
    x.v = b.template ld<3>(p + 3);
    return x;
}
template <class B> DSIM_FN DsimQuadSv<B> dq_sv_add(const B& b, const DsimQuadSv<B>& a, const DsimQuadSv<B>& x) {
    return DsimQuadSv<B>{b.add(a.w, x.w), b.add(a.v, x.v)};
}
template <class B> DSIM_FN DsimQuadSv<B> dq_unrot(const B& b, const DsimQuadSv<B>& t) {
    return DsimQuadSv<B>{b.template perm<DSIM_QP_YZXW>(t.w), b.template perm<DSIM_QP_YZXW>(t.v)};
}
template <class B> DSIM_FN DsimQuadSv<B> dq_unrot_add(const B& b, const DsimQuadSv<B>& acc, const DsimQuadSv<B>& t) {
    return DsimQuadSv<B>{b.add(acc.w, b.template perm<DSIM_QP_YZXW>(t.w)), b.add(acc.v, b.template perm<DSIM_QP_YZXW>(t.v))};
}
template <class B> DSIM_FN DsimQuadSv<B> dq_unrot_sub(const B& b, const DsimQuadSv<B>& acc, const DsimQuadSv<B>& t) {
    return DsimQuadSv<B>{b.sub(acc.w, b.template perm<DSIM_QP_YZXW>(t.w)), b.sub(acc.v, b.template perm<DSIM_QP_YZXW>(t.v))};
}
// S s and S s + y (joint motion: S_d qd_d; cotangent of S: aS + a_vj qd)
template <class B> DSIM_FN DsimQuadSv<B> dq_sv_scale(const B& b, const DsimQuadSv<B>& a, float s) {
    return DsimQuadSv<B>{dq_scale(b, a.w, s), dq_scale(b, a.v, s)};
}
template <class B> DSIM_FN DsimQuadSv<B> dq_sv_axpy(const B& b, const DsimQuadSv<B>& a, float s, const DsimQuadSv<B>& y) {
    return DsimQuadSv<B>{dq_axpy(b, a.w, s, y.w), dq_axpy(b, a.v, s, y.v)};
}
// spatial inertia from the 10 words (m, h, xx, xy, xz, yy, yz, zz) of dsim_math.hpp's inertia10
template <class B> DSIM_FN DsimQuadI<B> dq_ld_i10(const B& b, const float* p) {
    DsimQuadI<B> I;
    I.m = p[0];
    I.h = b.template ld<3>(p + 1);
    I.r0 = b.template ld_sym<0>(p + 4);
    I.r1 = b.template ld_sym<1>(p + 4);
    I.r2 = b.template ld_sym<2>(p + 4);
    return I;
}
// a x x for motion vectors (dsim_math.hpp: scross), rotated frame
template <class B> DSIM_FN DsimQuadSv<B> dq_scross_t(const B& b, const DsimQuadSv<B>& a, const DsimQuadSv<B>& x) {
    return DsimQuadSv<B>{dq_cross_t(b, a.w, x.w), dq_cross_t_acc(b, dq_cross_t(b, a.v, x.w), a.w, x.v)};
}
// a x* x (scross_dual), rotated frame; ... added to t
template <class B> DSIM_FN DsimQuadSv<B> dq_scross_dual_t(const B& b, const DsimQuadSv<B>& a, const DsimQuadSv<B>& x) {
    return DsimQuadSv<B>{dq_cross_t_acc(b, dq_cross_t(b, a.w, x.w), a.v, x.v), dq_cross_t(b, a.w, x.v)};
}
template <class B>
DSIM_FN DsimQuadSv<B> dq_scross_dual_t_acc(const B& b, const DsimQuadSv<B>& t, const DsimQuadSv<B>& a, const DsimQuadSv<B>& x) {
    return DsimQuadSv<B>{dq_cross_t_acc(b, dq_cross_t_acc(b, t.w, a.w, x.w), a.v, x.v), dq_cross_t_acc(b, t.v, a.w, x.v)};
}
// the cross-product pairs of f^T: cotangent of x in  y . (x x* f)  for a force f and a motion cotangent y -- written with the
// operands the way the phase has them,  (f.w x y.w + f.v x y.v,  f.v x y.w) = -(y x* f); rotated frame
template <class B> DSIM_FN DsimQuadSv<B> dq_fcross_t(const B& b, const DsimQuadSv<B>& f, const DsimQuadSv<B>& y) {
    return DsimQuadSv<B>{dq_cross_t_acc(b, dq_cross_t(b, f.w, y.w), f.v, y.v), dq_cross_t(b, f.v, y.w)};
}
// a . x of two spatial vectors, in components x, y, z (each lane adds the three pair products in its own cyclic order, dq_dot3)
template <class B> DSIM_FN typename B::T dq_sdot(const B& b, const DsimQuadSv<B>& a, const DsimQuadSv<B>& x) {
    const typename B::T p = b.fma(a.v, x.v, b.mul(a.w, x.w));
    return b.add(b.add(p, b.template perm<DSIM_QP_YZXW>(p)), b.template perm<DSIM_QP_ZXYW>(p));
}
// (a, 0) (x) x for a 3-vector a (dsim_math.hpp: qmul_v): dq_qmul without the term of a's w component, which is not read
template <class B> DSIM_FN typename B::T dq_qmul_v(const B& b, typename B::T a, typename B::T x) {
    typename B::T r = b.mul(b.mul(b.template perm<DSIM_QP_XYZX>(a), b.qs()), b.template perm<DSIM_QP_WWWX>(x));
    r = b.fma(b.mul(b.template perm<DSIM_QP_YZXY>(a), b.qs()), b.template perm<DSIM_QP_ZXYY>(x), r);
    return b.nfma(b.template perm<DSIM_QP_ZXYZ>(a), b.template perm<DSIM_QP_YZXZ>(x), r);
}
// ---- the free root's integrator and its adjoint (dsim_core.hpp: dsim_fwd_dynamics_wave, dsim_bwd_joint_wave) --------------------
// a . x of two quaternions, the same bits in all four components: the pair sums (x + y, z + w) first, then their sum -- an add
// is commutative, so (x + y) + (z + w) and (z + w) + (x + y) are one value
template <class B> DSIM_FN typename B::T dq_qdot(const B& b, typename B::T a, typename B::T x) {
    const typename B::T p = b.mul(a, x);
    const typename B::T s = b.add(p, b.template perm<DSIM_QP_YXWZ>(p));
    return b.add(s, b.template perm<DSIM_QP_ZWXY>(s));
}
// cotangent of the FIRST operand of a Hamilton product c = a (x) x for the cotangent g of c (dsim_math.hpp: qmul_adj_a):
// g (x) conj(x), conj's signs folded into the terms
template <class B> DSIM_FN typename B::T dq_qmul_adj_a(const B& b, typename B::T x, typename B::T g) {
    typename B::T r = b.mul(b.template perm<DSIM_QP_XYZX>(g), b.template perm<DSIM_QP_WWWX>(x));
    r = b.nfma(b.mul(b.template perm<DSIM_QP_WWWW>(g), b.qs()), x, r);
    r = b.nfma(b.mul(b.template perm<DSIM_QP_YZXY>(g), b.qs()), b.template perm<DSIM_QP_ZXYY>(x), r);
    return b.fma(b.template perm<DSIM_QP_ZXYZ>(g), b.template perm<DSIM_QP_YZXZ>(x), r);
}
// the identity quaternion (0, 0, 0, 1) from the sign constant (1, 1, 1, -1): 1/2 - qs / 2, exact
template <class B> DSIM_FN typename B::T dq_qident(const B& b) { return b.nfma(b.qs(), b.spl(0.5f), b.spl(0.5f)); }
// loads and stores of a 3-vector / quaternion by per-lane address (the quad backend's w lane stores nothing of a 3-vector)
template <class B> DSIM_FN typename B::T dq_ld3(const B& b, const float* p) { return b.template ld<3>(p); }
template <class B> DSIM_FN typename B::T dq_ldq(const B& b, const float* p) { return b.template ld<4>(p); }
template <class B> DSIM_FN void dq_st3(const B& b, float* p, typename B::T a) {
    if (b.xyz()) b.template st<3>(p, a);
}
template <class B> DSIM_FN void dq_stq(const B& b, float* p, typename B::T a) { b.template st<4>(p, a); }
// Semi-implicit Euler of a free joint (sim.py:1505-1636): w = qd_w + a_w h, vn = qd_v + a_v h, pn = p + (vn + w x p) h,
// rt = r + (w, 0) (x) r h / 2, rn = rt / |rt| -- the identity quaternion where |rt|^2 is below the smallest normal (il == 0;
// dsim_math.hpp: dsim_inv_len).  il rides in the checkpoint for integrate^T (dsim_core.hpp: DsimSavedIl).  The test on il is a
// select: all four lanes of a quad execute every permutation.
// The integrator keeps the roundings of its one-joint-per-lane form (dsim_math.hpp structs, as the compiler contracted them): the
// state after a step is the quantity a rollout feeds back 512 times, and environments that sit at a contact or joint-limit
// threshold follow another branch after a change in its last bit (tests/test_reference_episodes.py counts them).  Three places
// differ from the general forms above:
//   dq_qmul_v_int   the scalar part of (a, 0) (x) x summed in the order y, x, z (-(a_y x_y) rounded, the other two fused)
//   dq_qnorm2_int   |a|^2 as one chain y^2, + x^2, + z^2, + w^2 (four broadcasts) instead of the pair sums of dq_qdot
//   w x p           as -(p x w) through dq_cross_sub: the product that is rounded on its own is the second one
template <class B> DSIM_FN typename B::T dq_qmul_v_int(const B& b, typename B::T a, typename B::T x) {
    typename B::T r = b.mul(b.mul(b.template perm<DSIM_QP_XYZY>(a), b.qs()), b.template perm<DSIM_QP_WWWY>(x));
    r = b.fma(b.mul(b.template perm<DSIM_QP_YZXX>(a), b.qs()), b.template perm<DSIM_QP_ZXYX>(x), r);
    return b.nfma(b.template perm<DSIM_QP_ZXYZ>(a), b.template perm<DSIM_QP_YZXZ>(x), r);
}
template <class B> DSIM_FN typename B::T dq_qnorm2_int(const B& b, typename B::T a) {
    const typename B::T ax = b.template perm<DSIM_QP_XXXX>(a), ay = b.template perm<DSIM_QP_YYYY>(a);
    const typename B::T az = b.template perm<DSIM_QP_ZZZZ>(a), aw = b.template perm<DSIM_QP_WWWW>(a);
    return b.fma(aw, aw, b.fma(az, az, b.fma(ax, ax, b.mul(ay, ay))));
}
// (rt from r and w = qd_w + qdd_w h, and 1 / |rt|: integrate^T repeats the integrator's own expressions, rounding included)
template <class B> DSIM_FN typename B::T dq_root_rt(const B& b, typename B::T r, typename B::T w, float h) {
    return dq_axpy(b, dq_scale(b, dq_qmul_v_int(b, w, r), 0.5f), h, r);
}
template <class B> DSIM_FN float dq_root_il(const B& b, typename B::T rt) { return dsim_inv_len(b.any(dq_qnorm2_int(b, rt))); }
template <class B> struct DsimQuadRootStep {
    typename B::T pn, rn, w, vn;
    float il;
};
template <class B>
DSIM_FN DsimQuadRootStep<B> dq_root_integrate(const B& b, typename B::T p, typename B::T r, typename B::T qd_w, typename B::T qd_v,
                                              typename B::T a_w, typename B::T a_v, float h) {
    typedef typename B::T T;
    DsimQuadRootStep<B> o;
    o.w = dq_axpy(b, a_w, h, qd_w);
    o.vn = dq_axpy(b, a_v, h, qd_v);
    o.pn = dq_axpy(b, dq_cross_sub(b, o.vn, p, o.w), h, p);
    const T rt = dq_root_rt(b, r, o.w, h);
    o.il = dq_root_il(b, rt);
    o.rn = b.sel(o.il > 0.0f, dq_scale(b, rt, o.il), dq_qident(b));
    return o;
}
// integrate^T of the same update: cotangents g_pn, g_rn of the new pose and gqd_w, gqd_v of the new twist in; aq_p, aq_r: the
// cotangent of the old pose, g_w, g_v: that of the twist (w, vn).  il: the integrator's (0: the normalisation passed nothing)
template <class B> struct DsimQuadRootAdj {
    typename B::T aq_p, aq_r, g_w, g_v;
};
template <class B>
DSIM_FN DsimQuadRootAdj<B> dq_root_integrate_adj(const B& b, typename B::T p, typename B::T r, typename B::T w, typename B::T rt, float il,
                                                 typename B::T g_pn, typename B::T g_rn, typename B::T gqd_w, typename B::T gqd_v, float h) {
    typedef typename B::T T;
    DsimQuadRootAdj<B> o;
    const T rn = dq_scale(b, rt, il);
    const T g_rt = b.sel(il > 0.0f, dq_scale(b, b.nfma(rn, dq_qdot(b, rn, g_rn), g_rn), il), b.spl(0.f));
    const float hh = 0.5f * h;
    o.aq_r = b.nfma(dq_qmul_v(b, w, g_rt), b.spl(hh), g_rt);   // g_rt + conj(W) (x) g_rt h / 2, W = (w, 0)
    const T g_dp = dq_scale(b, g_pn, h);
    o.g_w = dq_cross_acc(b, dq_axpy(b, dq_qmul_adj_a(b, r, g_rt), hh, gqd_w), p, g_dp);
    o.g_v = b.add(g_dp, gqd_v);
    o.aq_p = dq_cross_sub(b, g_pn, w, g_dp);
    return o;
}

// Cotangent of a spatial inertia's 10 parameters (dsim_math.hpp: g[10]; the mass word is never needed).  The six words of the
// symmetric block are held as the three rows of G + G^T, G the cotangent of A's nine entries: the off-diagonal entries are the
// words themselves, the diagonal carries TWICE its word -- which is the matrix the pose wrench wants (dsim_core.hpp:
// inertia_pose_wrench, G2).  The first-moment part is h + (ht out of the rotated frame): ht collects cross products.  The body
// level only READS the cotangent from LDS (ai10m, dq_ld_g10) and consumes it as a pose wrench: no kernel stores this form.
template <class B> struct DsimQuadG {
    typename B::T h, ht, r0, r1, r2;
};
template <class B> DSIM_FN DsimQuadG<B> dq_g10_zero(const B& b) {
    const typename B::T z = b.spl(0.f);
    return DsimQuadG<B>{z, z, z, z, z};
}
template <class B> DSIM_FN DsimQuadG<B> dq_ld_g10(const B& b, const float* p) {
    DsimQuadG<B> g;
    g.h = b.template ld<3>(p + 1);
    g.ht = b.spl(0.f);
    const typename B::T r0 = b.template ld_sym<0>(p + 4), r1 = b.template ld_sym<1>(p + 4), r2 = b.template ld_sym<2>(p + 4);
    g.r0 = b.fma(r0, b.ex(), r0);
    g.r1 = b.fma(r1, b.ey(), r1);
    g.r2 = b.fma(r2, b.ez(), r2);
    return g;
}
// g += cotangent of y^T I x (dsim_math.hpp: inertia_bilinear_adj with weight 1):  G + G^T += y.w x.w^T + x.w y.w^T,
// g_h += x.v x y.w + y.v x x.w
template <class B> DSIM_FN void dq_inertia_bilinear_adj(const B& b, DsimQuadG<B>& g, const DsimQuadSv<B>& y, const DsimQuadSv<B>& x) {
    g.ht = dq_cross_t_acc(b, dq_cross_t_acc(b, g.ht, x.v, y.w), y.v, x.w);
    g.r0 = b.fma(y.w, b.template perm<DSIM_QP_XXXX>(x.w), b.fma(x.w, b.template perm<DSIM_QP_XXXX>(y.w), g.r0));
    g.r1 = b.fma(y.w, b.template perm<DSIM_QP_YYYY>(x.w), b.fma(x.w, b.template perm<DSIM_QP_YYYY>(y.w), g.r1));
    g.r2 = b.fma(y.w, b.template perm<DSIM_QP_ZZZZ>(x.w), b.fma(x.w, b.template perm<DSIM_QP_ZZZZ>(y.w), g.r2));
}
// g as a pose wrench (dsim_core.hpp: inertia_pose_wrench): torque = sum_k A_k x (G + G^T)_k + h x g_h over the rows k (rotated
// frame), force = tr(G + G^T) h - (G + G^T) h + m g_h.  A term u x grav of the gravity wrench joins g_h before the call
// (g.ht = dq_cross_t_acc(b, g.ht, u, grav)): both are h x . and m . of their sum.
template <class B> struct DsimQuadWrenchT {
    typename B::T wt, v;   // torque in the rotated frame, force
};
template <class B> DSIM_FN DsimQuadWrenchT<B> dq_inertia_pose_wrench(const B& b, const DsimQuadI<B>& I, const DsimQuadG<B>& g) {
    typedef typename B::T T;
    const T gh = b.add(g.h, b.template perm<DSIM_QP_YZXW>(g.ht));
    DsimQuadWrenchT<B> W;
    W.wt = dq_cross_t_acc(b, dq_cross_t_acc(b, dq_cross_t_acc(b, dq_cross_t(b, I.r0, g.r0), I.r1, g.r1), I.r2, g.r2), I.h, gh);
    const T d = b.fma(g.r2, b.ez(), b.fma(g.r1, b.ey(), b.mul(g.r0, b.ex())));
    const T tr = b.add(b.add(d, b.template perm<DSIM_QP_YZXW>(d)), b.template perm<DSIM_QP_ZXYW>(d));
    W.v = b.fma(gh, b.spl(I.m), b.sub(b.mul(I.h, tr), dq_sym_mul(b, g.r0, g.r1, g.r2, I.h)));
    return W;
}
