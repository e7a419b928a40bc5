// dsim_emu_kin.cpp -- TEST-ONLY: the differentiable kinematic read-out (dsim_core.hpp: dsim_body_kin_forward /
// dsim_body_kin_backward) on the lane-serial host executor of dsim_emu.cpp, generic and specialised layouts, one or four
// wavefronts per environment (dsim_emu_use_static / dsim_emu_set_waves of that file).  Included at the end of dsim_emu.cpp
// (one translation unit, tests/emu/Makefile); like that file it is not part of the library.  Null pointers mean what they mean in
// include/dsim.h (dsim_body_kinematics, dsim_body_kinematics_backward).
extern "C" int dsim_emu_body_kinematics(const dsim_model_desc* m, int n_envs, const float* q, const float* qd, float* xsc,
                                        float* xsm, float* vs) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    const size_t nq = lay.d.nq, nd = lay.d.nd, L = lay.d.L;
    return emu_each_env<false>(lay, n_envs, 1.0f, [&](auto& c, auto& ex, int e) {
        dsim_body_kin_forward(c, ex, q + e * nq, qd ? qd + e * nd : nullptr, xsc + e * 7 * L, xsm ? xsm + e * 7 * L : nullptr,
                              vs ? vs + e * 6 * L : nullptr);
    });
}

extern "C" int dsim_emu_body_kinematics_backward(const dsim_model_desc* m, int n_envs, const float* q, const float* qd,
                                                 const float* gxsc, const float* gxsm, const float* gvs, float* gq, float* gqd) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    const size_t nq = lay.d.nq, nd = lay.d.nd, L = lay.d.L;
    return emu_each_env<false>(lay, n_envs, 1.0f, [&](auto& c, auto& ex, int e) {
        dsim_body_kin_backward(c, ex, q + e * nq, qd ? qd + e * nd : nullptr, gxsc ? gxsc + e * 7 * L : nullptr,
                               gxsm ? gxsm + e * 7 * L : nullptr, gvs ? gvs + e * 6 * L : nullptr, gq + e * nq,
                               gqd ? gqd + e * nd : nullptr);
    });
}
