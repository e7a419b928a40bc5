// dsim_abi.hpp -- host side: the structs of the C ABI (include/dsim.h) -> the structs the phase code takes (dsim_core.hpp).
// The one statement of these field copies: the library (dsim_hip.hip, which validates the fields first) and the host harness
// of the tests (tests/emu/dsim_emu.cpp) both include it, so a field added to one side cannot be missed by the other.
// Include after dsim_core.hpp.
#pragma once

inline DsimEnvSpec dsim_env_spec_copy(const dsim_env_spec& e) {
    DsimEnvSpec sp;
    sp.kind = e.kind; sp.rew_kind = e.rew_kind; sp.n_act = e.n_act; sp.n_obs = e.n_obs;
    sp.act_offset = e.act_offset; sp.act_muscle = e.act_muscle; sp.obs_actions = e.obs_actions; sp.sanitize = e.sanitize_grads;
    for (int k = 0; k < 4; ++k) { sp.isr[k] = e.inv_start_rot[k]; sp.pen[k] = e.cartpole_penalties[k]; }
    sp.tgt_x = e.target_x; sp.tgt_z = e.target_z; sp.term_h = e.termination_height;
    sp.term_tol = e.termination_tolerance; sp.h_scale = e.height_rew_scale; sp.act_pen = e.action_penalty;
    sp.vel_scale = e.joint_vel_obs_scaling; sp.act_scale = e.act_scale;
    return sp;
}

inline DsimEpisode dsim_episode_copy(const dsim_episode& e) {
    DsimEpisode ep{};
    ep.progress = reinterpret_cast<long long*>(e.progress);
    ep.done = reinterpret_cast<long long*>(e.done);
    ep.obs_before = e.obs_before_reset;
    ep.reset_q = e.reset_q; ep.reset_qd = e.reset_qd; ep.reset_count = e.reset_count;
    ep.pool = e.reset_pool; ep.episode_length = e.episode_length;
    ep.height_terminate = e.height_terminate; ep.check_invalid = e.check_invalid;
    ep.noise_q = e.noise_q; ep.noise_qd = e.noise_qd; ep.noise_angle = e.noise_angle;
    ep.seed = e.seed;
    return ep;
}
