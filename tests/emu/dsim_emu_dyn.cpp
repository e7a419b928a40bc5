// dsim_emu_dyn.cpp -- TEST-ONLY: the differentiable dynamic read-out (dsim_core.hpp: dsim_joint_dyn_forward /
// dsim_joint_dyn_backward) on the lane-serial host executor of dsim_emu.cpp, generic and specialised layouts, one or four
// wavefronts per environment (dsim_emu_use_static / dsim_emu_set_waves of that file).  Included at the end of dsim_emu.cpp
// (one translation unit, tests/emu/Makefile); like that file it is not part of the library.  Null pointers mean what they mean in
// include/dsim.h (dsim_joint_dynamics, dsim_joint_dynamics_backward).
extern "C" int dsim_emu_joint_dynamics(const dsim_model_desc* m, int n_envs, const float* q, const float* qd, const float* act,
                                       const float* mact, float* tau, float* qdd, float* fs) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    const size_t nq = lay.d.nq, nd = lay.d.nd, L = lay.d.L, M = lay.d.M;
    return emu_each_env<false>(lay, n_envs, 1.0f, [&](auto& c, auto& ex, int e) {
        dsim_joint_dyn_forward(c, ex, q + e * nq, qd + e * nd, act ? act + e * nd : nullptr, (mact && M) ? mact + e * M : nullptr,
                               tau ? tau + e * nd : nullptr, qdd ? qdd + e * nd : nullptr, fs ? fs + e * 6 * L : nullptr);
    });
}

extern "C" int dsim_emu_joint_dynamics_backward(const dsim_model_desc* m, int n_envs, const float* q, const float* qd,
                                                const float* act, const float* mact, const float* gtau, const float* gqdd,
                                                const float* gfs, float* gq, float* gqd, float* gact, float* gmact) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    const size_t nq = lay.d.nq, nd = lay.d.nd, L = lay.d.L, M = lay.d.M;
    return emu_each_env<false>(lay, n_envs, 1.0f, [&](auto& c, auto& ex, int e) {
        dsim_joint_dyn_backward(c, ex, q + e * nq, qd + e * nd, act ? act + e * nd : nullptr, (mact && M) ? mact + e * M : nullptr,
                                gtau ? gtau + e * nd : nullptr, gqdd ? gqdd + e * nd : nullptr, gfs ? gfs + e * 6 * L : nullptr,
                                gq + e * nq, gqd + e * nd, gact ? gact + e * nd : nullptr, (gmact && M) ? gmact + e * M : nullptr);
    });
}
