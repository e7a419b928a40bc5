// dsim_emu_kin.cpp -- TEST-ONLY: the differentiable kinematic read-out (dsim_core.hpp: dsim_body_kin_forward /
// dsim_body_kin_backward) on the lane-serial host executor of dsim_emu.cpp, generic and specialised layouts, one or four
// wavefronts per environment (dsim_emu_use_static / dsim_emu_set_waves of that file).  Built by tests/kin_emu_lib.py with the
// flags of tests/emu/Makefile; like dsim_emu.cpp it is not part of the library.  Null pointers mean what they mean in
// include/dsim.h (dsim_body_kinematics, dsim_body_kinematics_backward).
#include "dsim_emu.cpp"

extern "C" int dsim_emu_body_kinematics(const dsim_model_desc* m, int n_envs, const float* q, const float* qd, float* xsc,
                                        float* xsm, float* vs) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    const size_t nq = lay.d.nq, nd = lay.d.nd, L = lay.d.L;
    return emu_dispatch(lay, [&](auto o, auto d, auto& ex, auto) {
        for (int e = 0; e < n_envs; ++e) {
            std::vector<float> lds(lay.o.total_words, 0.f);
            memcpy(lds.data(), lay.cblob.data(), sizeof(uint32_t) * lay.o.const_words);
            DsimCtxT<decltype(o), decltype(d), false> c;
            c.s = lds.data(); c.k = c.s; c.o = o; c.d = d; c.h = 1.0f;
            dsim_body_kin_forward(c, ex, q + e * nq, qd ? qd + e * nd : nullptr, xsc + e * 7 * L, xsm ? xsm + e * 7 * L : nullptr,
                                  vs ? vs + e * 6 * L : nullptr);
        }
        return 0;
    });
}

extern "C" int dsim_emu_body_kinematics_backward(const dsim_model_desc* m, int n_envs, const float* q, const float* qd,
                                                 const float* gxsc, const float* gxsm, const float* gvs, float* gq, float* gqd) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    const size_t nq = lay.d.nq, nd = lay.d.nd, L = lay.d.L;
    return emu_dispatch(lay, [&](auto o, auto d, auto& ex, auto) {
        for (int e = 0; e < n_envs; ++e) {
            std::vector<float> lds(lay.o.total_words, 0.f);
            memcpy(lds.data(), lay.cblob.data(), sizeof(uint32_t) * lay.o.const_words);
            DsimCtxT<decltype(o), decltype(d), false> c;
            c.s = lds.data(); c.k = c.s; c.o = o; c.d = d; c.h = 1.0f;
            dsim_body_kin_backward(c, ex, q + e * nq, qd ? qd + e * nd : nullptr, gxsc ? gxsc + e * 7 * L : nullptr,
                                   gxsm ? gxsm + e * 7 * L : nullptr, gvs ? gvs + e * 6 * L : nullptr, gq + e * nq,
                                   gqd ? gqd + e * nd : nullptr);
        }
        return 0;
    });
}
