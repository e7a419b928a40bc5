// dsim_emu_con.cpp -- TEST-ONLY: the differentiable ground-contact read-out (dsim_core.hpp: dsim_ground_contact_forward /
// dsim_ground_contact_backward) on the lane-serial host executor of dsim_emu.cpp, generic and specialised layouts, one or four
// wavefronts per environment (dsim_emu_use_static / dsim_emu_set_waves of that file).  Included at the end of dsim_emu.cpp
// (one translation unit, tests/emu/Makefile); like that file it is not part of the library.  Null pointers mean what they mean in
// include/dsim.h (dsim_ground_contacts, dsim_ground_contacts_backward).
extern "C" int dsim_emu_ground_contacts(const dsim_model_desc* m, int n_envs, const float* q, const float* qd, float* point,
                                        float* vel, float* force, float* lw) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    const size_t nq = lay.d.nq, nd = lay.d.nd, L = lay.d.L, Cn = lay.d.C;
    return emu_each_env<false>(lay, n_envs, 1.0f, [&](auto& c, auto& ex, int e) {
        dsim_ground_contact_forward(c, ex, q + e * nq, qd + e * nd, point ? point + e * 3 * Cn : nullptr,
                                    vel ? vel + e * 3 * Cn : nullptr, force ? force + e * 3 * Cn : nullptr,
                                    lw ? lw + e * 6 * L : nullptr);
    });
}

extern "C" int dsim_emu_ground_contacts_backward(const dsim_model_desc* m, int n_envs, const float* q, const float* qd,
                                                 const float* gpoint, const float* gvel, const float* gforce, const float* glw,
                                                 float* gq, float* gqd) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    const size_t nq = lay.d.nq, nd = lay.d.nd, L = lay.d.L, Cn = lay.d.C;
    return emu_each_env<false>(lay, n_envs, 1.0f, [&](auto& c, auto& ex, int e) {
        dsim_ground_contact_backward(c, ex, q + e * nq, qd + e * nd, gpoint ? gpoint + e * 3 * Cn : nullptr,
                                     gvel ? gvel + e * 3 * Cn : nullptr, gforce ? gforce + e * 3 * Cn : nullptr,
                                     glw ? glw + e * 6 * L : nullptr, gq + e * nq, gqd + e * nd);
    });
}
