// dsim_emu_jac.cpp -- TEST-ONLY: the step Jacobian (dsim_core.hpp: dsim_multi_slot around dsim_sim_step_backward) on the
// lane-serial host executor of dsim_emu.cpp, generic and specialised layouts, one or four wavefronts per environment, full or
// lean checkpoints (dsim_emu_use_static / dsim_emu_set_waves / dsim_emu_set_ckpt_lean of that file).  Included at the end
// of dsim_emu.cpp (one translation unit, tests/emu/Makefile); like that file it is not part of the library.  The entry points walk the block
// indices of the device launch, 0 .. n_envs * n_cot - 1, and take every pointer from dsim_multi_slot -- the code the kernels
// run; the single sweep with its own per-environment pointer arithmetic, as dsim_bwd_kernel does it, is dsim_emu_step_backward
// of dsim_emu.cpp.

// the device launch of dsim_bwd_multi_kernel, block by block
static int jac_run_multi(const DsimLayout& lay, int n_envs, float dt, int substeps, int mm_freq, DsimMultiArgs a) {
    a.ckpt_stride = (long long)dsim_ckpt_words(emu_row(lay), lay.d.nq, lay.d.nd, substeps, mm_freq);
    return emu_each_env(lay, n_envs * a.n_cot, dt / float(substeps), [&](auto& c, auto& ex, int b) {
        const DsimMultiSlot s = dsim_multi_slot(a, b, c.d.nd, c.d.M);
        dsim_sim_step_backward(c, ex, substeps, mm_freq, s.ckpt, s.act, s.mact, s.gq_out, s.gqd_out, s.gq_in, s.gqd_in, s.gact,
                               s.gmact);
    });
}

extern "C" int dsim_emu_step_backward_multi(const dsim_model_desc* m, int n_envs, int n_cot, int cot_shared, const float* ckpt,
                                            const float* act, const float* mact, float dt, int substeps, int mm_freq,
                                            const float* gq_out, const float* gqd_out, float* gq_in, float* gqd_in, float* gact,
                                            float* gmact) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    const int nq = lay.d.nq, nd = lay.d.nd, M = lay.d.M;
    DsimMultiArgs a{};
    a.n_cot = n_cot; a.cot_shared = cot_shared != 0;
    a.ckpt = ckpt; a.act = act; a.mact = mact;
    a.gq_out = gq_out; a.gqd_out = gqd_out; a.gq_out_stride = nq; a.gqd_out_stride = nd;
    a.gq_in = gq_in; a.gqd_in = gqd_in; a.gact = gact; a.gmact = gmact;
    a.gq_in_stride = nq; a.gqd_in_stride = nd; a.gact_stride = nd; a.gmact_stride = M;
    return jac_run_multi(lay, n_envs, dt, substeps, mm_freq, a);
}

extern "C" int dsim_emu_step_jacobian(const dsim_model_desc* m, int n_envs, const float* ckpt, const float* act, const float* mact,
                                      float dt, int substeps, int mm_freq, float* J_state, float* J_act, float* J_muscle) {
    DsimLayout lay;
    if (!dsim_build_layout(*m, lay).empty()) return -1;
    const int nq = lay.d.nq, nd = lay.d.nd, M = lay.d.M, K = nq + nd;
    std::vector<float> eye((size_t)K * K, 0.f);
    for (int i = 0; i < K; ++i) eye[(size_t)i * K + i] = 1.0f;
    DsimMultiArgs a{};
    a.n_cot = K; a.cot_shared = 1;
    a.ckpt = ckpt; a.act = act; a.mact = mact;
    a.gq_out = eye.data(); a.gqd_out = eye.data() + nq; a.gq_out_stride = K; a.gqd_out_stride = K;
    a.gq_in = J_state; a.gqd_in = J_state + nq; a.gact = J_act; a.gmact = J_muscle;
    a.gq_in_stride = K; a.gqd_in_stride = K; a.gact_stride = nd; a.gmact_stride = M;
    return jac_run_multi(lay, n_envs, dt, substeps, mm_freq, a);
}
