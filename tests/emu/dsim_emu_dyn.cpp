// dsim_emu_dyn.cpp -- TEST-ONLY: the differentiable dynamic read-out (dsim_core.hpp: dsim_joint_dyn_forward /
// dsim_joint_dyn_backward) on the lane-serial host executor of dsim_emu.cpp, generic and specialised layouts, one or four
// wavefronts per environment (dsim_emu_use_static / dsim_emu_set_waves of that file).  Built by tests/dyn_lib.py with the
// flags of tests/emu/Makefile; like dsim_emu.cpp it is not part of the library.  Null pointers mean what they mean in
// include/dsim.h (dsim_joint_dynamics, dsim_joint_dynamics_backward).
#include "dsim_emu.cpp"

extern "C" int dsim_emu_joint_dynamics(const dsim_model_desc* m, int n_envs, const float* q, const float* qd, const float* act,
                                       const float* mact, float* tau, float* qdd, float* fs) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    const size_t nq = lay.d.nq, nd = lay.d.nd, L = lay.d.L, M = lay.d.M;
    return emu_dispatch(lay, [&](auto o, auto d, auto& ex, auto) {
        for (int e = 0; e < n_envs; ++e) {
            std::vector<float> lds(lay.o.total_words, 0.f);
            memcpy(lds.data(), lay.cblob.data(), sizeof(uint32_t) * lay.o.const_words);
            DsimCtxT<decltype(o), decltype(d), false> c;
            c.s = lds.data(); c.k = c.s; c.o = o; c.d = d; c.h = 1.0f;
            dsim_joint_dyn_forward(c, ex, q + e * nq, qd + e * nd, act ? act + e * nd : nullptr, (mact && M) ? mact + e * M : nullptr,
                                   tau ? tau + e * nd : nullptr, qdd ? qdd + e * nd : nullptr, fs ? fs + e * 6 * L : nullptr);
        }
        return 0;
    });
}

extern "C" int dsim_emu_joint_dynamics_backward(const dsim_model_desc* m, int n_envs, const float* q, const float* qd,
                                                const float* act, const float* mact, const float* gtau, const float* gqdd,
                                                const float* gfs, float* gq, float* gqd, float* gact, float* gmact) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    const size_t nq = lay.d.nq, nd = lay.d.nd, L = lay.d.L, M = lay.d.M;
    return emu_dispatch(lay, [&](auto o, auto d, auto& ex, auto) {
        for (int e = 0; e < n_envs; ++e) {
            std::vector<float> lds(lay.o.total_words, 0.f);
            memcpy(lds.data(), lay.cblob.data(), sizeof(uint32_t) * lay.o.const_words);
            DsimCtxT<decltype(o), decltype(d), false> c;
            c.s = lds.data(); c.k = c.s; c.o = o; c.d = d; c.h = 1.0f;
            dsim_joint_dyn_backward(c, ex, q + e * nq, qd + e * nd, act ? act + e * nd : nullptr, (mact && M) ? mact + e * M : nullptr,
                                    gtau ? gtau + e * nd : nullptr, gqdd ? gqdd + e * nd : nullptr, gfs ? gfs + e * 6 * L : nullptr,
                                    gq + e * nq, gqd + e * nd, gact ? gact + e * nd : nullptr, (gmact && M) ? gmact + e * M : nullptr);
        }
        return 0;
    });
}
