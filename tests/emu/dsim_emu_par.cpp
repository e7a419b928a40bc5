// dsim_emu_par.cpp -- TEST-ONLY: the step adjoint with model-parameter gradients (dsim_core.hpp: DsimParCtxT around
// dsim_sim_step_backward; the device form is dsim_bwd_param_kernel) on the lane-serial host executor of dsim_emu.cpp, generic and
// specialised layouts, one or four wavefronts per environment, full or lean checkpoints (dsim_emu_use_static / dsim_emu_set_waves /
// dsim_emu_set_ckpt_lean of that file).  A translation unit of its own that includes the harness; tests/par_lib.py builds it with
// the flags of tests/emu/Makefile.  Like dsim_emu.cpp it is not part of the library.
//
// `params`: NULL, or six pointers in the order of the DSIM_PARAM_* fields of include/dsim.h (target_ke, target_kd, limit_ke,
// limit_kd, target, contact_material), each NULL or an array that replaces the template's in the constant block -- the host form
// of dsim_model_set_params, a copy into the block at the field's layout offset.
#include "dsim_emu.cpp"

#include <limits>

static void par_apply(DsimLayout& lay, const float* const* params) {
    if (!params) return;
    const DsimOff& o = lay.o;
    const DsimDims& d = lay.d;
    const int off[6] = {o.tke, o.tkd, o.lke, o.lkd, o.target, o.cmat};
    const int n[6] = {d.L, d.L, d.L, d.L, d.nq, 4 * d.C};
    for (int f = 0; f < 6; ++f)
        if (params[f] && n[f] > 0) memcpy(lay.cblob.data() + off[f], params[f], sizeof(float) * (size_t)n[f]);
}

extern "C" int dsim_emu_par_forward(const dsim_model_desc* m, const float* const* params, int n_envs, const float* q_in,
                                    const float* qd_in, const float* act, const float* mact, float dt, int substeps, int mm_freq,
                                    float* q_out, float* qd_out, float* ckpt) {
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

// g_dof [n_envs][5][nd], g_contact [n_envs][C][4]; with BOTH null the sweep runs on the plain context: dsim_step_backward itself
extern "C" int dsim_emu_par_backward(const dsim_model_desc* m, const float* const* params, int n_envs, const float* ckpt,
                                     const float* act, const float* mact, float dt, int substeps, int mm_freq, const float* gq_out,
                                     const float* gqd_out, float* gq_in, float* gqd_in, float* gact, float* gmact, float* g_dof,
                                     float* g_contact) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    par_apply(lay, params);
    const size_t nq = lay.d.nq, nd = lay.d.nd, M = lay.d.M, C = lay.d.C;
    const size_t stride = dsim_ckpt_words(emu_row(lay), lay.d.nq, lay.d.nd, substeps, mm_freq);
    const float h = dt / float(substeps);
    if (!g_dof && !g_contact)
        return emu_each_env(lay, n_envs, h, [&](auto& c, auto& ex, int e) {
            dsim_sim_step_backward(c, ex, substeps, mm_freq, ckpt + e * stride, act + e * nd, M ? mact + e * M : nullptr,
                                   gq_out + e * nq, gqd_out + e * nd, gq_in + e * nq, gqd_in + e * nd, gact ? gact + e * nd : nullptr,
                                   (gmact && M) ? gmact + e * M : nullptr);
        });
    // the accumulators start as NaN: the sweep itself must clear them, as the kernel must clear its LDS words
    std::vector<float> acc;
    return emu_each_env(lay, n_envs, h, [&](auto& c0, auto& ex, int e) {
        using Base = std::decay_t<decltype(c0)>;
        DsimParCtxT<decltype(c0.o), decltype(c0.d), Base::LEAN> c;
        static_cast<Base&>(c) = c0;
        acc.assign((size_t)dsim_par_words((int)nd, (int)C), std::numeric_limits<float>::quiet_NaN());
        c.pg = acc.data();
        c.g_dof = g_dof ? g_dof + e * 5 * nd : nullptr;
        c.g_contact = (g_contact && C) ? g_contact + e * 4 * C : nullptr;
        dsim_sim_step_backward(c, ex, substeps, mm_freq, ckpt + e * stride, act + e * nd, M ? mact + e * M : nullptr,
                               gq_out + e * nq, gqd_out + e * nd, gq_in + e * nq, gqd_in + e * nd, gact ? gact + e * nd : nullptr,
                               (gmact && M) ? gmact + e * M : nullptr);
    });
}
