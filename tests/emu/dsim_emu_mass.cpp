// dsim_emu_mass.cpp -- TEST-ONLY: the differentiable mass matrix read-out (dsim_core.hpp: dsim_mass_forward / dsim_mass_backward)
// on the lane-serial host executor of dsim_emu.cpp, generic and specialised layouts, one or four wavefronts per environment
// (dsim_emu_use_static / dsim_emu_set_waves of that file).  Included at the end of dsim_emu.cpp (one translation unit,
// tests/emu/Makefile); like that file it is not part of the library.  Null pointers mean what they mean in include/dsim.h
// (dsim_mass_matrix, dsim_mass_matrix_backward).
extern "C" int dsim_emu_mass_matrix(const dsim_model_desc* m, int n_envs, const float* q, float* H, float* Hinv, float* S) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    const size_t nq = lay.d.nq, nd = lay.d.nd;
    return emu_each_env<false>(lay, n_envs, 1.0f, [&](auto& c, auto& ex, int e) {
        dsim_mass_forward(c, ex, q + e * nq, H ? H + e * nd * nd : nullptr, Hinv ? Hinv + e * nd * nd : nullptr,
                          S ? S + e * 6 * nd : nullptr);
    });
}

extern "C" int dsim_emu_mass_matrix_backward(const dsim_model_desc* m, int n_envs, const float* q, const float* gH,
                                             const float* gHinv, const float* gS, float* gq) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    const size_t nq = lay.d.nq, nd = lay.d.nd;
    return emu_each_env<false>(lay, n_envs, 1.0f, [&](auto& c, auto& ex, int e) {
        dsim_mass_backward(c, ex, q + e * nq, gH ? gH + e * nd * nd : nullptr, gHinv ? gHinv + e * nd * nd : nullptr,
                           gS ? gS + e * 6 * nd : nullptr, gq + e * nq);
    });
}
