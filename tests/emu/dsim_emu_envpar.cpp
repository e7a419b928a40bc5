// dsim_emu_envpar.cpp -- TEST-ONLY: the host harness (dsim_emu.cpp, every entry point of it) plus the fused env step under given
// parameter values and its adjoint with the model-parameter gradients: dsim_env_fused_backward on DsimParCtxT, the host form of
// dsim_env_bwd_param_kernel (dsim_env_step_backward_params).  Built as libdsim_emu_envpar.so (tests/emu/GNUmakefile).
#include "dsim_emu.cpp"

// dsim_emu_env_forward with `params` (six pointers as in dsim_emu_step_forward, or NULL) copied into the constant block first
extern "C" int dsim_emu_env_forward_params(const dsim_model_desc* m, const float* const* params, const dsim_env_spec* env, int n_envs,
                                           const float* q_in, const float* qd_in, const float* actions, float dt, int substeps,
                                           int mm_freq, float* q_out, float* qd_out, float* obs, float* rew, float* ckpt,
                                           const dsim_episode* episode) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    par_apply(lay, params);
    const int nq = lay.d.nq, nd = lay.d.nd;
    DsimEnvSpec sp = dsim_env_spec_copy(*env);
    DsimEpisode ep = episode ? dsim_episode_copy(*episode) : DsimEpisode{};
    const size_t stride = dsim_ckpt_words(emu_row(lay), nq, nd, substeps, mm_freq);
    return emu_each_env(lay, n_envs, dt / float(substeps), [&](auto& c, auto& ex, int e) {
        dsim_env_fused_forward(c, ex, sp, substeps, mm_freq, q_in + (size_t)e * nq, qd_in + (size_t)e * nd,
                               actions + (size_t)e * sp.n_act, q_out + (size_t)e * nq, qd_out + (size_t)e * nd,
                               obs + (size_t)e * sp.n_obs, rew + e, ckpt ? ckpt + (size_t)e * stride : nullptr, ep, e, n_envs);
    });
}

// g_dof [n_envs][5][nd], g_contact [n_envs][C][4], either may be null; ALWAYS on the parameter context, as the kernel is
extern "C" int dsim_emu_env_backward_params(const dsim_model_desc* m, const float* const* params, const dsim_env_spec* env,
                                            int n_envs, const float* ckpt, const float* actions, float dt, int substeps, int mm_freq,
                                            const float* gq_out, const float* gqd_out, const float* gobs, const float* grew,
                                            const float* gobs_before, float* gq_in, float* gqd_in, float* gactions, float* g_dof,
                                            float* g_contact) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    par_apply(lay, params);
    const size_t nq = lay.d.nq, nd = lay.d.nd, C = lay.d.C;
    DsimEnvSpec sp = dsim_env_spec_copy(*env);
    const size_t stride = dsim_ckpt_words(emu_row(lay), lay.d.nq, lay.d.nd, substeps, mm_freq);
    std::vector<float> acc;
    return emu_each_env(lay, n_envs, dt / float(substeps), [&](auto& c0, auto& ex, int e) {
        using Base = std::decay_t<decltype(c0)>;
        DsimParCtxT<decltype(c0.o), decltype(c0.d), Base::LEAN> c;
        static_cast<Base&>(c) = c0;
        // the accumulators start as NaN: the driver itself must clear them, as the kernel must clear its LDS words
        acc.assign((size_t)dsim_par_words((int)nd, (int)C), std::numeric_limits<float>::quiet_NaN());
        c.pg = acc.data();
        c.g_dof = g_dof ? g_dof + e * 5 * nd : nullptr;
        c.g_contact = (g_contact && C) ? g_contact + e * 4 * C : nullptr;
        dsim_env_fused_backward(c, ex, sp, substeps, mm_freq, ckpt + e * stride, actions + e * sp.n_act,
                                gq_out ? gq_out + e * nq : nullptr, gqd_out ? gqd_out + e * nd : nullptr,
                                gobs ? gobs + e * sp.n_obs : nullptr, grew ? grew + e : nullptr,
                                gobs_before ? gobs_before + e * sp.n_obs : nullptr, gq_in + e * nq, gqd_in + e * nd,
                                gactions + e * sp.n_act);
    });
}
