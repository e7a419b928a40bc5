// dsim_emu.cpp -- TEST-ONLY harness: runs the kernel phase code of diffrl_amd/csrc/dsim_core.hpp with a
// lane-serial executor on the host so that the phase logic (indexing, adjoint algebra) can be
// unit-tested in the GPU-less build container.  It is NOT a CPU fallback: nothing in diffrl_amd/
// loads it, and it is built only by tests/emu/Makefile.  The GPU tests (-m gpu) exercise the real
// HIP kernels through the C ABI.
#include <ucontext.h>

#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <vector>

#define DSIM_FN static inline
#include "../../diffrl_amd/csrc/dsim_core.hpp"
#include "../../diffrl_amd/csrc/dsim_abi.hpp"
#include "../../diffrl_amd/csrc/dsim_literal.hpp"
#ifdef DSIM_STATIC_LAYOUTS_FILE   // (a generated header with user models: tests/inject/dsim_static_layouts_user.hpp, see the Makefile)
#include DSIM_STATIC_LAYOUTS_FILE
#else
#include "../../diffrl_amd/csrc/dsim_static_layouts.hpp"
#endif

// NW wavefronts per environment: NL = 64 * NW lanes (the library's kernels use 1 or 4).
//
// One wavefront (NW == 1): the lanes of a phase run as 64 coroutines in lock step, so that the phase code may use the
// wavefront's cross-lane primitives -- shfl (ds_bpermute on the GPU), bcast (v_readlane), lds_fence -- exactly where the
// kernels use them: a lane that reaches a collective deposits its value and yields; once every lane still running has
// arrived, each continues with the value of its source lane.  Four wavefronts: plain lane-serial execution, no
// cross-lane primitives (the kernels have none across wavefronts either; WAVE_OPS is false).
// LANES == 32: the lane count the phase code sees when TWO environments share a wavefront (dsim_hip.hip: DSIM_MODE_PAIR,
// DevExec EPW == 2) -- every variant choice that depends on Exec::NL is then the pair kernels'.
template <int NW, int LANES = DSIM_NL> struct HostExecT {
    static constexpr int NL = LANES * NW;
    static constexpr bool WAVE_OPS = NW == 1;
    static constexpr size_t STACK = 512 * 1024;
    ucontext_t main_ctx_, lane_ctx_[NL];
    std::vector<char> stacks_;
    std::function<void(int)> body_;
    bool done_[NL];
    int cur_ = 0, parity_[NL];
    float slot_[2][NL];
    static HostExecT*& self() {
        static thread_local HostExecT* p = nullptr;
        return p;
    }
    static void tramp(int lane) {
        HostExecT* e = self();
        e->body_(lane);
        e->done_[lane] = true;
        swapcontext(&e->lane_ctx_[lane], &e->main_ctx_);
    }
    // the first `n` lanes as lock-step coroutines (cross-lane primitives allowed inside f)
    template <class F> void run_coro(F&& f, int n) {
        if (stacks_.size() < STACK * (size_t)n) stacks_.resize(STACK * (size_t)n);
        body_ = [&f](int lane) { f(lane); };
        self() = this;
        for (int lane = 0; lane < n; ++lane) {
            done_[lane] = false;
            parity_[lane] = 0;
            getcontext(&lane_ctx_[lane]);
            lane_ctx_[lane].uc_stack.ss_sp = stacks_.data() + STACK * lane;
            lane_ctx_[lane].uc_stack.ss_size = STACK;
            lane_ctx_[lane].uc_link = &main_ctx_;
            makecontext(&lane_ctx_[lane], (void (*)())tramp, 1, lane);
        }
        for (int left = n; left > 0;) {
            left = 0;
            for (int lane = 0; lane < n; ++lane) {
                if (done_[lane]) continue;
                cur_ = lane;
                swapcontext(&main_ctx_, &lane_ctx_[lane]);  // runs until the lane's next collective or its end
                if (!done_[lane]) ++left;
            }
        }
    }
    template <class F> void run(F&& f) {
        if constexpr (!WAVE_OPS) {
            for (int lane = 0; lane < NL; ++lane) f(lane);
        } else {
            run_coro(f, NL);
        }
    }
    // a phase of the environment's FIRST wavefront alone (device: DevExec::run_wave0), with its cross-lane primitives
    static constexpr bool WAVE0_OPS = true;
    template <class F> void run_wave0(F&& f) { run_coro(f, LANES); }
    // collectives (only meaningful inside run(), NW == 1).  Every lane that is still running must call the same sequence.
    void arrive() {
        const int lane = cur_;
        swapcontext(&lane_ctx_[lane], &main_ctx_);  // back to the scheduler; resumed when all running lanes have arrived
    }
    float shfl(float v, int src) {
        const int lane = cur_, p = parity_[lane];
        slot_[p][lane] = v;
        parity_[lane] ^= 1;
        arrive();
        return slot_[p][src & (NL - 1)];
    }
    float bcast(float v, int src) { return shfl(v, src); }
    // DPP row shift of the device executor: lane + D of the same 16-lane row, 0 beyond the row's end
    template <int D> float from_above(float v) {
        const int lane = cur_, src = lane + D;
        const float r = shfl(v, src < LANES ? src : lane);
        return (src < LANES && (src >> 4) == (lane >> 4)) ? r : 0.f;
    }
    template <int D> float from_below(float v) {
        const int lane = cur_, src = lane - D;
        const float r = shfl(v, src >= 0 ? src : lane);
        return (src >= 0 && (src >> 4) == (lane >> 4)) ? r : 0.f;
    }
    template <bool FIRST = true> void add_from_next(float& a0, float& a1, float& a2, float& a3, float& a4, float& a5, float w) {
        const int lane = cur_;
        auto nx = [&](float v) { const float r = shfl(v, lane + 1 < LANES ? lane + 1 : lane); return lane + 1 < LANES ? r : 0.f; };
        const float y0 = nx(a0), y1 = nx(a1), y2 = nx(a2), y3 = nx(a3), y4 = nx(a4), y5 = nx(a5);
        a0 = __builtin_fmaf(y0, w, a0); a1 = __builtin_fmaf(y1, w, a1); a2 = __builtin_fmaf(y2, w, a2);
        a3 = __builtin_fmaf(y3, w, a3); a4 = __builtin_fmaf(y4, w, a4); a5 = __builtin_fmaf(y5, w, a5);
    }
    template <int SRC> void add_from_lane(float& a0, float& a1, float& a2, float& a3, float& a4, float& a5, float w) {
        const float s0 = bcast(a0, SRC), s1 = bcast(a1, SRC), s2 = bcast(a2, SRC), s3 = bcast(a3, SRC), s4 = bcast(a4, SRC), s5 = bcast(a5, SRC);
        a0 = __builtin_fmaf(s0, w, a0); a1 = __builtin_fmaf(s1, w, a1); a2 = __builtin_fmaf(s2, w, a2);
        a3 = __builtin_fmaf(s3, w, a3); a4 = __builtin_fmaf(s4, w, a4); a5 = __builtin_fmaf(s5, w, a5);
    }
    void loads_landed() {}
    void group_sync() {}                                       // (no helper wavefront here: DsimHelperCommit is off)
    void helper_prefetch(const float*, int) {}
    void helper_commit(float*, int, const float*) {}
    void helper_prefetch_aux(const float*, int) {}
    void helper_commit_aux(float*, float*, int) {}
    template <int D, bool FIRST = true> void add_from_above(float& a0, float& a1, float& a2, float& a3, float& a4, float& a5, float w) {
        const float y0 = from_above<D>(a0), y1 = from_above<D>(a1), y2 = from_above<D>(a2), y3 = from_above<D>(a3),
                    y4 = from_above<D>(a4), y5 = from_above<D>(a5);
        a0 = __builtin_fmaf(y0, w, a0); a1 = __builtin_fmaf(y1, w, a1); a2 = __builtin_fmaf(y2, w, a2);
        a3 = __builtin_fmaf(y3, w, a3); a4 = __builtin_fmaf(y4, w, a4); a5 = __builtin_fmaf(y5, w, a5);
    }
    void lds_fence() { arrive(); }
    void system_fence() {}
    template <class F> void fire(F&& f) { run(f); }
    // the helper wavefront of the device executor (dsim_hip.hip) does not exist here: both blocks of a split phase run in
    // the one emulated wave, one after the other
    static constexpr bool HAS_HELPER = false;
    template <class F> void run_both(F&& f) { run(f); }
    template <class FM, class FH> void fork_join(FM&& fm, FH&& fh) {
        run([&](int lane) {
            fm(lane);
            fh(lane);
        });
    }
    // fm hands over to fh at its mid() call (device: the helper's barrier): every lane passes mid() before any lane gets to fh
    template <class FM, class FH> void fork_join_mid(FM&& fm, FH&& fh) { fork_join(fm, fh); }
    template <class FM, class FH> void fork_mid_detached(FM&& fm, FH&& fh) { fork_join(fm, fh); }
    // Several wavefronts (device: DevExec::fork_wave0): the first wavefront's lanes and the others' run as coroutines of one group;
    // mid() / mid2() / side_done_w() are WORKGROUP BARRIERS there -- no lane passes one before every lane of the group has reached
    // it -- while the first wavefront's cross-lane primitives (shfl, lds_fence) stay lock-step points of its own lanes only (the
    // other lanes' blocks use none).
    int bar_n_ = 0, bar_cnt_ = 0, bar_gen_ = 0;
    void wbar() {
        const int gen = bar_gen_;
        if (++bar_cnt_ == bar_n_) {
            bar_cnt_ = 0;
            ++bar_gen_;
        }
        do arrive();
        while (bar_gen_ == gen);
    }
    template <class F0, class FR> void fork_wave0(F0&& f0, FR&& fr) {
        static_assert(NW > 1, "fork_wave0 belongs to the mapping with several wavefronts per environment");
        bar_n_ = NL;
        bar_cnt_ = 0;
        in_coro_ = true;
        run_coro([&](int lane) {
            if (lane < LANES) f0(lane);
            else fr(lane - LANES);
        }, NL);
        in_coro_ = false;
        bar_n_ = 0;
    }
    void mid() {
        if (bar_n_) wbar();
        else arrive();
    }
    void mid2() {
        if (bar_n_) wbar();
    }
    void side_done_w() { wbar(); }
    // side block first, then the main block, whose side_done() is a point every lane passes (device: the helper's barrier)
    template <class FM, class FH> void fork_side(FM&& fm, FH&& fh) {
        run([&](int lane) {
            fh(lane);
            arrive();
            fm(lane);
        });
    }
    void side_done() { arrive(); }
    void stamp() {}
    // host form of the register / v_readlane Gauss-Jordan of the kernels (dsim_hip.hip: dsim_wave_gj, deferred scaling of the
    // pivot rows): same formulas in the same order (the device's pivot reciprocal is v_rcp_f32 + a Newton step, here 1 / x)
    template <int N> void wave_gj(float* H) {
        float scale[N];
        for (int i = 0; i < N; ++i) scale[i] = 1.0f;
        for (int k = 0; k < N; ++k) {
            const float rp = 1.0f / H[k * N + k];
            float f[N];
            for (int i = 0; i < N; ++i) f[i] = (i == k) ? 0.0f : H[i * N + k] * rp;
            scale[k] = rp;
            for (int i = 0; i < N; ++i) H[i * N + k] = (i == k) ? 1.0f : 0.0f;
            float hk[N];
            for (int j = 0; j < N; ++j) hk[j] = H[k * N + j];
            for (int i = 0; i < N; ++i)
                for (int j = 0; j < N; ++j) H[i * N + j] = __builtin_fmaf(-f[i], hk[j], H[i * N + j]);
        }
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) H[i * N + j] *= scale[i];
    }
    static constexpr bool WAVE_GJ_PAD = true;
    template <int NB> void wave_gj_pad(float* H, int n) {   // (device: the matrix padded with an identity block in registers)
        float P[NB * NB];
        for (int i = 0; i < NB; ++i)
            for (int j = 0; j < NB; ++j) P[i * NB + j] = (i < n && j < n) ? H[i * n + j] : (i == j ? 1.0f : 0.0f);
        wave_gj<NB>(P);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) H[i * n + j] = P[i * NB + j];
    }
    void mark(int) {}
    void begin_request() {}
    void begin() {}   // the host image is set up by emu_ctx (constants copied, work area zero)
    float io_[NL][DSIM_IO_MAX];   // early-load registers of the specialised kernels
    float* io(int lane) { return io_[lane]; }
    float hacc_[NL][DSIM_HACC_MAX];  // what a lane keeps in registers across phases on the GPU
    float* hacc(int lane) { return hacc_[lane]; }
    float hpf_[NL][DSIM_HPF_MAX];
    float* hpf(int lane) { return hpf_[lane]; }
    DsimTopoRegs topo_[NL];
    DsimTopoRegs& topo(int lane) { return topo_[lane]; }
    const float* pf_src = nullptr;
    void prefetch(const float* row, int) { pf_src = row; }
    void commit(float* dst, int words, int lane) {
        for (int k = lane; k < words; k += NL) dst[k] = pf_src[k];
    }
    // (per lane: on the device the row waits in each lane's own registers; here a lane of fork_wave0's second block requests the
    // row after the next while the lanes behind it have not committed theirs yet)
    const float* pf_rest_[NL] = {};
    bool in_coro_ = false;
    void prefetch_rest(const float* row, int) {
        if (in_coro_) pf_rest_[cur_] = row;
        else for (int l = 0; l < NL; ++l) pf_rest_[l] = row;
    }
    void commit_rest(float* dst, int words, int lane) {
        for (int k = lane; k < words; k += NL - LANES) dst[k] = pf_rest_[lane + LANES][k];
    }
};
typedef HostExecT<1> HostExec;

// DSIM_EMU_EXECUTOR_ONLY: the executor alone, without the entry points below and their instantiations of the phase code (the
// check programs of tests/quad, which drive the phase code's quad primitives on a HostExec themselves)
#ifndef DSIM_EMU_EXECUTOR_ONLY
static int g_lean = 0;   // checkpoint mode of the emu entry points (dsim_model_set_ckpt_mode of the library)
extern "C" void dsim_emu_set_ckpt_lean(int on) { g_lean = on; }
static int emu_row(const DsimLayout& lay) { return g_lean ? lay.o.xsc - lay.o.q : lay.o.save_words; }
static int g_waves = 1;
extern "C" void dsim_emu_set_waves(int w) { g_waves = w > 1 ? 4 : 1; }
static int g_half = 0;   // 32 lanes per environment (specialised one-wave variants only: the pair kernels)
extern "C" void dsim_emu_set_half_wave(int on) { g_half = on; }

// The image of one environment on the host: zeros with the model constants copied in (what DevExec::begin leaves in LDS), and
// the context of the given layout types and checkpoint mode on it.  The one statement of this prologue: every entry point gets
// its context here -- those that run the kernels' variants through emu_each_env below, the operator-level ones in front of it
// (always the generic one-wave path, whatever the mode switches say) directly.
template <bool LEAN = false, class O, class D>
static DsimCtxT<O, D, LEAN> emu_ctx(const DsimLayout& lay, std::vector<float>& lds, float h, O o, D d) {
    lds.assign(lay.o.total_words, 0.f);
    memcpy(lds.data(), lay.cblob.data(), sizeof(uint32_t) * lay.o.const_words);
    DsimCtxT<O, D, LEAN> c;
    c.s = lds.data(); c.k = c.s; c.o = o; c.d = d; c.h = h;
    return c;
}
static DsimCtx emu_ctx(const DsimLayout& lay, std::vector<float>& lds, float h) { return emu_ctx(lay, lds, h, lay.o, lay.d); }

extern "C" {

int dsim_emu_layout(const dsim_model_desc* m, int* off_out, int n_off, int* dims_out) {
    DsimLayout lay;
    std::string err = dsim_build_layout(*m, lay);
    if (!err.empty()) return -1;
    const int n = (int)(sizeof(DsimOff) / sizeof(int));
    if (n_off < n) return n;
    memcpy(off_out, &lay.o, sizeof(DsimOff));
    memcpy(dims_out, &lay.d, sizeof(DsimDims));
    return n;
}

// one substep (with mass-matrix refresh) for ONE env; returns the LDS image for inspection
int dsim_emu_substep_image(const dsim_model_desc* m, const float* q, const float* qd, const float* act,
                           const float* mact, float h, float* image) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    std::vector<float> lds;
    DsimCtx c = emu_ctx(lay, lds, h);
    memcpy(lds.data() + lay.o.q, q, 4 * lay.d.nq);
    memcpy(lds.data() + lay.o.qd, qd, 4 * lay.d.nd);
    memcpy(lds.data() + lay.o.act, act, 4 * lay.d.nd);
    if (lay.d.M) memcpy(lds.data() + lay.o.mact, mact, 4 * lay.d.M);
    HostExec ex;
    dsim_fwd_kinematics(c, ex);
    dsim_fwd_external(c, ex);
    dsim_fwd_tau(c, ex);
    dsim_fwd_mass(c, ex);
    dsim_fwd_solve(c, ex);
    memcpy(image, lds.data(), 4 * lay.o.total_words);
    return 0;
}
}

// dsim_step_backward_literal on the host: the adjoint phases with the export of (gq_1, gqd_1, adj H), then the forward-mode
// tangent of the first substep (diffrl_amd/csrc/dsim_literal.hpp) link by link, exactly what dsim_literal_radial_kernel does
extern "C" int dsim_emu_step_backward_literal(const dsim_model_desc* m, int n_envs, const float* ckpt, const float* act,
                                              const float* mact, float dt, int substeps, int mm_freq, const float* gq_out,
                                              const float* gqd_out, float* gq_in, float* gqd_in, float* gact, float* gmact,
                                              float* lit_out) {   // lit_out: [n_envs][nq + nd + nd * nd] or null (tests)
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    const int nq = lay.d.nq, nd = lay.d.nd, M = lay.d.M, L = lay.d.L;
    if (L > DSIM_LIT_LMAX || nd > DSIM_LIT_NDMAX) return -4;
    HostExec ex;
    const size_t stride = dsim_ckpt_words(lay.o.save_words, nq, nd, substeps, mm_freq);
    std::vector<float> lit((size_t)nq + nd + (size_t)nd * nd);
    dsim_lit::Consts cc;
    cc.cb = lay.cblob.data();
    cc.o = lay.o;
    cc.d = lay.d;
    for (int e = 0; e < n_envs; ++e) {
        std::vector<float> lds;
        DsimCtx c = emu_ctx(lay, lds, dt / float(substeps));
        const float* row = ckpt + (size_t)e * stride;
        dsim_sim_step_backward(c, ex, substeps, mm_freq, row, act + (size_t)e * nd, M ? mact + (size_t)e * M : nullptr,
                               gq_out + (size_t)e * nq, gqd_out + (size_t)e * nd, gq_in + (size_t)e * nq, gqd_in + (size_t)e * nd,
                               gact ? gact + (size_t)e * nd : nullptr, (gmact && M) ? gmact + (size_t)e * M : nullptr, lit.data());
        const float* hinv = row + (size_t)substeps * lay.o.save_words;
        if (lit_out) memcpy(lit_out + (size_t)e * lit.size(), lit.data(), sizeof(float) * lit.size());
        for (int i = 0; i < L; ++i) {
            const int type = cc.I(lay.o.jtype, i);
            if (type != DSIM_JOINT_BALL && type != DSIM_JOINT_FREE) continue;
            const float rho = dsim_lit::radial(cc, row, row + (lay.o.qd - lay.o.q), act + (size_t)e * nd, M ? mact + (size_t)e * M : nullptr,
                                               dt / float(substeps), hinv, lit.data(), lit.data() + nq, lit.data() + nq + nd, i);
            const int qs = cc.I(lay.o.qstart, i) + (type == DSIM_JOINT_FREE ? 3 : 0);
            for (int j = 0; j < 4; ++j) gq_in[(size_t)e * nq + qs + j] += rho * row[qs + j];
        }
    }
    return 0;
}

// test helper: tangents (d tau [nd], d qdd [nd], d H [nd][nd]) of the first substep along the radial direction of link `jl`'s quaternion
extern "C" int dsim_emu_literal_tangents(const dsim_model_desc* m, const float* q, const float* qd, const float* act, const float* mact,
                                         float h, const float* hinv, int jl, float* out, const float* lit, float* rho_out) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    const int nq = lay.d.nq, nd = lay.d.nd;
    dsim_lit::Consts cc;
    cc.cb = lay.cblob.data();
    cc.o = lay.o;
    cc.d = lay.d;
    std::vector<float> z((size_t)nq + nd + (size_t)nd * nd, 0.f);
    for (int k = 0; k < 2 * nd + nd * nd; ++k) out[k] = 0.f;
    const float* l = lit ? lit : z.data();
    const float rho = dsim_lit::radial(cc, q, qd, act, mact, h, hinv, l, l + nq, l + nq + nd, jl, out);
    if (rho_out) *rho_out = rho;
    return 0;
}

// ---- fused env surface (host lane-serial) ----
// The per-model specialised code paths (compile-time layouts: `if constexpr (DsimIsStatic...)` branches, bounded sums)
// can be exercised on the host too: with dsim_emu_use_static(1) the env entry points below instantiate the phase code
// with the generated all-constexpr layout of the matching model, exactly as the library's dispatch() does.
static int g_use_static = 0;
extern "C" void dsim_emu_use_static(int on) { g_use_static = on; }

template <class F, class O, class D> static int emu_waves(F&& f, O o, D d) {
    if (g_waves > 1) {
        static HostExecT<4> ex4;
        return g_lean ? f(o, d, ex4, std::true_type{}) : f(o, d, ex4, std::false_type{});
    }
    if constexpr (dsim_pair_ok<D>()) {
        if (g_half) {
            static HostExecT<1, 32> exh;
            return g_lean ? f(o, d, exh, std::true_type{}) : f(o, d, exh, std::false_type{});
        }
    }
    if (g_half) return -3;   // no pair kernels for this model
    static HostExecT<1> ex1;
    return g_lean ? f(o, d, ex1, std::true_type{}) : f(o, d, ex1, std::false_type{});
}
template <class F> static int emu_dispatch(const DsimLayout& lay, F&& f) {
    if (!g_use_static) return emu_waves(f, lay.o, lay.d);
    const size_t no = sizeof(DsimOff) / sizeof(int), nd = sizeof(DsimDims) / sizeof(int);
#define DSIM_EMU_CASE(T)                                                                                            \
    if (sizeof(kDsimStatic##T) == (no + nd) * sizeof(int) && memcmp(kDsimStatic##T, &lay.o, no * sizeof(int)) == 0 && \
        memcmp(kDsimStatic##T + no, &lay.d, nd * sizeof(int)) == 0)                                                  \
        return emu_waves(f, DsimOff##T{}, DsimDims##T{});
    DSIM_STATIC_VARIANTS(DSIM_EMU_CASE)
#undef DSIM_EMU_CASE
    return -2;  // no specialised variant for this model
}

// f(c, ex, e) for e = 0 .. n_envs - 1 with a fresh image each (emu_ctx) in the layout types, wave count and checkpoint mode the
// switches above select -- the host form of "one environment per workgroup".  CKPT_MODES = false: an entry point without checkpoints
// (the read-outs, which have no lean variant on the device either) always gets the full-checkpoint context.
template <bool CKPT_MODES = true, class F> static int emu_each_env(const DsimLayout& lay, int n_envs, float h, F&& f) {
    return emu_dispatch(lay, [&](auto o, auto d, auto& ex, auto lean) {
        std::vector<float> lds;
        for (int e = 0; e < n_envs; ++e) {
            auto c = emu_ctx<CKPT_MODES && decltype(lean)::value>(lay, lds, h, o, d);
            f(c, ex, e);
        }
        return 0;
    });
}

// ---- the step: forward and adjoint sweep, one environment after the other ----
// `params`: NULL, or six pointers in the order of the DSIM_PARAM_* fields of include/dsim.h (target_ke, target_kd, limit_ke,
// limit_kd, target, contact_material), each NULL or an array that replaces the template's in the constant block -- the host form
// of dsim_model_set_params, a copy into the block at the field's layout offset.
static void par_apply(DsimLayout& lay, const float* const* params) {
    if (!params) return;
    const DsimOff& o = lay.o;
    const DsimDims& d = lay.d;
    const int off[6] = {o.tke, o.tkd, o.lke, o.lkd, o.target, o.cmat};
    const int n[6] = {d.L, d.L, d.L, d.L, d.nq, 4 * d.C};
    for (int f = 0; f < 6; ++f)
        if (params[f] && n[f] > 0) memcpy(lay.cblob.data() + off[f], params[f], sizeof(float) * (size_t)n[f]);
}

extern "C" int dsim_emu_step_forward(const dsim_model_desc* m, const float* const* params, int n_envs, const float* q_in,
                                     const float* qd_in, const float* act, const float* mact, float dt, int substeps, int mm_freq,
                                     float* q_out, float* qd_out, float* ckpt) {   // ckpt: null = no checkpoints
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    par_apply(lay, params);
    const size_t nq = lay.d.nq, nd = lay.d.nd, M = lay.d.M;
    const size_t stride = dsim_ckpt_words(emu_row(lay), lay.d.nq, lay.d.nd, substeps, mm_freq);
    return emu_each_env(lay, n_envs, dt / float(substeps), [&](auto& c, auto& ex, int e) {
        dsim_sim_step_forward(c, ex, substeps, mm_freq, q_in + e * nq, qd_in + e * nd, act + e * nd, M ? mact + e * M : nullptr,
                              q_out + e * nq, qd_out + e * nd, ckpt ? ckpt + e * stride : nullptr);
    });
}

// g_dof [n_envs][5][nd], g_contact [n_envs][C][4]: the model-parameter gradients (dsim_core.hpp: DsimParCtxT around
// dsim_sim_step_backward; the device form is dsim_bwd_param_kernel).  With BOTH null the sweep runs on the plain context:
// dsim_step_backward itself, the pointer arithmetic of dsim_bwd_kernel.
extern "C" int dsim_emu_step_backward(const dsim_model_desc* m, const float* const* params, int n_envs, const float* ckpt,
                                      const float* act, const float* mact, float dt, int substeps, int mm_freq, const float* gq_out,
                                      const float* gqd_out, float* gq_in, float* gqd_in, float* gact, float* gmact, float* g_dof,
                                      float* g_contact) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    par_apply(lay, params);
    const size_t nq = lay.d.nq, nd = lay.d.nd, M = lay.d.M, C = lay.d.C;
    const size_t stride = dsim_ckpt_words(emu_row(lay), lay.d.nq, lay.d.nd, substeps, mm_freq);
    const bool with_params = g_dof || g_contact;
    std::vector<float> acc;
    return emu_each_env(lay, n_envs, dt / float(substeps), [&](auto& c0, auto& ex, int e) {
        auto sweep = [&](auto& c) {
            dsim_sim_step_backward(c, ex, substeps, mm_freq, ckpt + e * stride, act + e * nd, M ? mact + e * M : nullptr,
                                   gq_out + e * nq, gqd_out + e * nd, gq_in + e * nq, gqd_in + e * nd, gact ? gact + e * nd : nullptr,
                                   (gmact && M) ? gmact + e * M : nullptr);
        };
        if (!with_params) return sweep(c0);
        using Base = std::decay_t<decltype(c0)>;
        DsimParCtxT<decltype(c0.o), decltype(c0.d), Base::LEAN> c;
        static_cast<Base&>(c) = c0;
        // the accumulators start as NaN: the sweep itself must clear them, as the kernel must clear its LDS words
        acc.assign((size_t)dsim_par_words((int)nd, (int)C), std::numeric_limits<float>::quiet_NaN());
        c.pg = acc.data();
        c.g_dof = g_dof ? g_dof + e * 5 * nd : nullptr;
        c.g_contact = (g_contact && C) ? g_contact + e * 4 * C : nullptr;
        sweep(c);
    });
}

extern "C" int dsim_emu_env_forward(const dsim_model_desc* m, const dsim_env_spec* env, int n_envs, const float* q_in,
                                    const float* qd_in, const float* actions, float dt, int substeps, int mm_freq,
                                    float* q_out, float* qd_out, float* obs, float* rew, float* ckpt,
                                    const dsim_episode* episode) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    const int nq = lay.d.nq, nd = lay.d.nd;
    DsimEnvSpec sp = dsim_env_spec_copy(*env);
    DsimEpisode ep = episode ? dsim_episode_copy(*episode) : DsimEpisode{};
    const size_t stride = dsim_ckpt_words(emu_row(lay), nq, nd, substeps, mm_freq);
    return emu_each_env(lay, n_envs, dt / float(substeps), [&](auto& c, auto& ex, int e) {
        dsim_env_fused_forward(c, ex, sp, substeps, mm_freq, q_in + (size_t)e * nq, qd_in + (size_t)e * nd,
                               actions + (size_t)e * sp.n_act, q_out + (size_t)e * nq, qd_out + (size_t)e * nd,
                               obs + (size_t)e * sp.n_obs, rew + e, ckpt ? ckpt + (size_t)e * stride : nullptr, ep, e,
                               n_envs);
    });
}

extern "C" int dsim_emu_env_backward(const dsim_model_desc* m, const dsim_env_spec* env, int n_envs, const float* ckpt,
                                     const float* actions, float dt, int substeps, int mm_freq, const float* gq_out,
                                     const float* gqd_out, const float* gobs, const float* grew,
                                     const float* gobs_before, float* gq_in, float* gqd_in, float* gactions) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    const int nq = lay.d.nq, nd = lay.d.nd;
    DsimEnvSpec sp = dsim_env_spec_copy(*env);
    const size_t stride = dsim_ckpt_words(emu_row(lay), nq, nd, substeps, mm_freq);
    return emu_each_env(lay, n_envs, dt / float(substeps), [&](auto& c, auto& ex, int e) {
        dsim_env_fused_backward(c, ex, sp, substeps, mm_freq, ckpt + (size_t)e * stride,
                                actions + (size_t)e * sp.n_act, gq_out ? gq_out + (size_t)e * nq : nullptr,
                                gqd_out ? gqd_out + (size_t)e * nd : nullptr,
                                gobs ? gobs + (size_t)e * sp.n_obs : nullptr, grew ? grew + e : nullptr,
                                gobs_before ? gobs_before + (size_t)e * sp.n_obs : nullptr, gq_in + (size_t)e * nq,
                                gqd_in + (size_t)e * nd, gactions + (size_t)e * sp.n_act);
    });
}

extern "C" long long dsim_emu_ckpt_floats(const dsim_model_desc* m, int substeps, int mm_freq) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    return dsim_ckpt_words(emu_row(lay), lay.d.nq, lay.d.nd, substeps, mm_freq);
}

// the read-outs and the step Jacobian: entry points of the same harness, kept in files of their own
#include "dsim_emu_kin.cpp"
#include "dsim_emu_dyn.cpp"
#include "dsim_emu_jac.cpp"
#include "dsim_emu_mass.cpp"
#include "dsim_emu_con.cpp"
#endif   // DSIM_EMU_EXECUTOR_ONLY
