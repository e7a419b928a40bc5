/* dsim.h -- C ABI of the MI355X-native differentiable articulated rigid-body step.
 *
 * This is the drop-in boundary for the hot path of NVlabs/DiffRL's dflex:
 *
 *   dsim_step_forward   replaces  SimulateFunc.forward  (dflex/dflex/sim.py:2097-2123), i.e. the
 *                       `substeps` calls of SemiImplicitIntegrator._simulate (sim.py:2225-2601)
 *                       that one SemiImplicitIntegrator.forward (sim.py:2182-2221) performs:
 *                       eval_rigid_fk, eval_rigid_id, eval_rigid_contacts_art, eval_muscles,
 *                       eval_rigid_tau, eval_rigid_jacobian, eval_rigid_mass,
 *                       eval_dense_gemm_batched x2, eval_dense_cholesky_batched,
 *                       eval_dense_solve_batched, eval_rigid_integrate
 *   dsim_step_backward  replaces  SimulateFunc.backward (sim.py:2127-2154) + Tape.replay
 *                       (dflex/dflex/adjoint.py:2153-2199): the reverse sweep over the same launches
 *   dsim_model_create   replaces  the tensors ModelBuilder.finalize + Model.collide upload
 *                       (dflex/dflex/model.py:1646-1879, 424-515) -- but ONE articulation template
 *                       shared by all environments instead of N replicated copies
 *
 * Conventions (same as the reference FFI, dflex/dflex/adjoint.py:1250-1289, where noted):
 *   - plain pointers + sizes; device pointers are borrowed for the duration of the call;
 *   - all floating point is IEEE fp32, indices int32;
 *   - state tensors are environment-major: q[N][n_q], qd[N][n_qd], act[N][n_qd],
 *     muscle_act[N][n_muscles]  (== the reference's flat joint_q.view(N, -1));
 *   - spatial_transform = (px,py,pz, qx,qy,qz,qw); spatial_vector = (wx,wy,wz, vx,vy,vz);
 *     6x6 inertia row-major, rotational block upper-left (dflex/dflex/util.py:340-349);
 *   - kernels are enqueued on the caller's HIP stream, no host synchronisation inside;
 *   - gradients are WRITTEN (not accumulated) -- unlike the reference (adjoint.h:335-347) the
 *     caller does not need to zero them;
 *   - every function returns DSIM_OK or a negative error code; dsim_last_error() gives the text.
 *     (The reference has no error returns: with_pytorch_error_handling=False, adjoint.py:1875.)
 */
#ifndef DSIM_H
#define DSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSIM_OK 0
#define DSIM_ERR_INVALID (-1)   /* bad argument / unsupported model */
#define DSIM_ERR_HIP (-2)       /* HIP runtime error */
#define DSIM_ERR_LIMIT (-3)     /* model exceeds a compiled-in limit */

/* joint types, dflex/dflex/model.py:26-31 */
#define DSIM_JOINT_PRISMATIC 0
#define DSIM_JOINT_REVOLUTE 1
#define DSIM_JOINT_BALL 2
#define DSIM_JOINT_FIXED 3
#define DSIM_JOINT_FREE 4

/* One articulation ("environment") template. All pointers are HOST pointers and are copied. */
typedef struct dsim_model_desc {
    int32_t n_links;      /* L */
    int32_t n_q;          /* generalized coordinates per articulation */
    int32_t n_qd;         /* degrees of freedom per articulation */
    int32_t n_contacts;   /* static ground-contact points (Model.collide) ; 0 if ground is off */
    int32_t n_muscles;    /* M */
    int32_t n_waypoints;  /* W = muscle_start[M] */
    const int32_t* joint_type;      /* [L] */
    const int32_t* joint_parent;    /* [L]  -1 = world; parents precede children */
    const int32_t* joint_q_start;   /* [L+1] */
    const int32_t* joint_qd_start;  /* [L+1] */
    const float* joint_X_pj;        /* [L][7] joint frame in parent */
    const float* joint_X_cm;        /* [L][7] body COM frame in child (rotation is identity) */
    const float* joint_axis;        /* [L][3] */
    const float* body_I_m;          /* [L][36] spatial inertia at the COM */
    const float* joint_armature;    /* [n_qd] */
    const float* joint_target;      /* [n_q] */
    const float* joint_target_ke;   /* [L] */
    const float* joint_target_kd;   /* [L] */
    const float* joint_limit_lower; /* [n_q] */
    const float* joint_limit_upper; /* [n_q] */
    const float* joint_limit_ke;    /* [L] */
    const float* joint_limit_kd;    /* [L] */
    const int32_t* contact_body;    /* [C] */
    const float* contact_point;     /* [C][3] */
    const float* contact_dist;      /* [C] */
    const float* contact_material;  /* [C][4] (ke, kd, kf, mu) already gathered per contact */
    const int32_t* muscle_start;    /* [M+1] */
    const int32_t* muscle_links;    /* [W] */
    const float* muscle_points;     /* [W][3] */
    float gravity[3];
} dsim_model_desc;

typedef struct dsim_model dsim_model; /* opaque, owns device copies of the template */

/* Admitted models -- the one statement of the envelope (DESIGN.md "Admitted models" has the reasons; tests/big_models.py
 * builds a model at every edge of it).  dsim_model_create accepts an articulation with
 *   1 <= n_links <= 64, 1 <= n_qd <= 64, 1 <= n_q <= 96   (DSIM_ERR_INVALID beyond, "n_links must be in [1,64]" ...; with the
 *                        five joint kinds 64 dofs reach at most 85 coordinates, so n_q never binds on its own),
 *   any count of contacts, muscles and way-points whose LDS image of one environment -- constants, forward and adjoint work
 *                        arrays -- is at most 160 KiB = 163,840 bytes (DSIM_ERR_LIMIT beyond),
 *   joints of the five kinds above, parents before children, a block-diagonal body_I_m, an unrotated joint_X_cm.
 * Such a model runs every call below on the generic (run-time layout) kernels, or on a kernel set compiled for it, except:
 *   dsim_step_backward_literal   n_links <= 24 and n_qd <= 28 (DSIM_ERR_LIMIT beyond; dsim_step_backward has no such limit),
 *   dsim_step_backward_params    LDS image + 4 * (5 * n_qd + 4 * n_contacts) bytes <= 160 KiB (DSIM_ERR_LIMIT beyond;
 *                                dsim_step_backward still works),
 *   dsim_step_backward_multi, dsim_step_jacobian   n_envs * n_cot <= 2^24 - 1 workgroups in one call
 *                                (DSIM_ERR_LIMIT beyond; dsim_step_jacobian: n_cot = n_q + n_qd). */

const char* dsim_last_error(void);
int dsim_version(void);

/* Uploads the template to the CURRENT HIP device; the model belongs to that device from then on.  One process may hold
 * models on several GPUs ("one stream (or process) per GPU"): every call that takes a model must be
 * made with the model's device current (hipSetDevice / torch.cuda.device), with a stream and pointers of that device, and
 * returns DSIM_ERR_INVALID otherwise -- a launch on another device would read a constant block that is not there. */
int dsim_model_create(const dsim_model_desc* desc, dsim_model** out);
int dsim_model_destroy(dsim_model* m);
int dsim_model_device(const dsim_model* m);   /* HIP device index the model was created on */
/* 0: generic kernels (runtime layout); > 0: a per-model specialised kernel set is in use (layout matched a
 * compile-time table exactly).  Same results either way. */
int dsim_model_variant(const dsim_model* m);
/* Wavefronts per environment of this model's kernels: 1, or 4 for a model with more than 64 ground contacts or more than 64
 * active muscle segments (the generic kernels: DSIM_WAVES=1|4 in the environment at dsim_model_create overrides the choice).
 * Same results either way. */
int dsim_model_waves(const dsim_model* m);

/* Floats per environment of the checkpoint the forward launch leaves in HBM for the adjoint launch: per
 * substep one "saved block" (q, qd and the forward intermediates the adjoint reads: transforms, motion
 * subspace, twists, inertias, subtree forces, accelerations) plus one inverse mass matrix per refresh.
 * (The reference keeps all 14 State tensors of every substep alive on its Tape, sim.py:2111 /
 * model.py:338-392.)  dsim_ckpt_floats() is the upper bound over mm_freq (mm_freq = 1). */
int64_t dsim_ckpt_floats_mm(const dsim_model* m, int substeps, int mm_freq);

/* Checkpoint mode of a model (default DSIM_CKPT_FULL).  Affects dsim_ckpt_floats(_mm) and every later forward / backward
 * call with a checkpoint; a checkpoint must be consumed in the mode it was written in.
 *   DSIM_CKPT_FULL  one row per substep with everything the adjoint reads (q, qd, X_sc, S, v, a, world inertias, f_tot,
 *                   qdd): the adjoint launch reads it back instead of recomputing it (fastest; HBM is idle on this path).
 *                   Floats per environment and env-step: Ant 7,524 (30 KB), Humanoid 49,748 (199 KB), SNUHumanoid
 *                   33,272 (133 KB), i.e. 0.99 / 6.5 / 2.2 GB for a 1024- (SNU: 512-) environment, H = 32 rollout.
 *   DSIM_CKPT_LEAN  one row per substep with (q, qd) only + the inverse mass matrices: the adjoint launch recomputes the
 *                   forward phases of every substep (same code, bit-identical intermediates, identical gradients).
 *                   Ant 740 floats (3 KB), Humanoid 3,476 (14 KB), SNUHumanoid 6,200 (25 KB) per environment and env-step:
 *                   for rollouts whose full checkpoint would not fit (tens of thousands of environments per GPU). */
#define DSIM_CKPT_FULL 0
#define DSIM_CKPT_LEAN 1
int dsim_model_set_ckpt_mode(dsim_model* m, int mode);
int64_t dsim_ckpt_floats(const dsim_model* m, int substeps);

/* One env.step() worth of simulation for N environments: `substeps` semi-implicit substeps of
 * dt/substeps with joint_act / muscle_act held fixed; mass matrix + Cholesky factor refreshed on
 * substeps i with i % mm_freq == 0 (sim.py:2113).
 *   ckpt: [N][dsim_ckpt_floats_mm(m, substeps, mm_freq)] or NULL (no-grad fast path == dflex.config.no_grad,
 *   sim.py:2201); every row starts with the (q, qd) entering its substep
 *   muscle_act may be NULL when n_muscles == 0.  q_out/qd_out may alias q_in/qd_in.
 *
 * PRECONDITION -- THE PATH IS DEFINED ON UNIT QUATERNIONS ONLY, FORWARD AND ADJOINT.  Every quaternion block of q_in (free
 * joint: q[cs+3 .. cs+6], ball joint: q[cs .. cs+3]) must be a unit quaternion to 1e-4.  The reference evaluates its rotation
 * formulas literally off the manifold (quat.h:113-116 rotate, spatial.h:559-586 / sim.py:1117-1134 T^T I_m T with a
 * non-orthogonal R); this library uses forms that agree with them ON the manifold only (10-parameter rigid-body inertia, pose
 * cotangents as wrenches).  Measured on the Ant step recording with the root quaternion scaled (host harness vs the
 * reference-order oracle): |q| = 1.001 -> 5.3e-3 relative error in qd_out, 1.01 -> 4.7e-2, 1.1 -> 0.64, against the 1e-4
 * state tolerance on the manifold.  States produced by the path itself always qualify: the integrator renormalises every
 * quaternion in every substep (sim.py:1552, 1616), so only states a caller constructs (reset_with_state, hand-made inputs)
 * can violate this.
 * ENFORCEMENT: the forward kernels check the state as loaded, once per launch; | |q|^2 - 1 | > 2e-4 in any block of any
 * environment marks the model, and the NEXT dsim_* call that takes the model returns DSIM_ERR_INVALID (once; the mark is
 * cleared) instead of launching -- asynchronous, like the error of a HIP kernel, no synchronisation on the step path.
 * dsim_model_status() asks explicitly (synchronise the stream first for a definitive answer about launches in flight). */
int dsim_step_forward(const dsim_model* m, int n_envs,
                      const float* q_in, const float* qd_in, const float* act, const float* muscle_act,
                      float dt, int substeps, int mm_freq,
                      float* q_out, float* qd_out, float* ckpt, void* hip_stream);

/* DSIM_OK, or DSIM_ERR_INVALID if a forward launch since the last report was handed a non-unit quaternion (see the
 * precondition above); *first_env (may be NULL) receives an environment index that saw one, -1 otherwise.  Reads two words
 * of host memory the kernels write to; never touches a stream.  Reporting clears the mark. */
int dsim_model_status(dsim_model* m, int* first_env);

/* Reverse sweep of the same step.  Needs the checkpoint of the forward call and the same act /
 * muscle_act.  Outputs: gq_in[N][n_q], gqd_in[N][n_qd], gact[N][n_qd], gmuscle_act[N][M]
 * (gact / gmuscle_act may be NULL to skip).  Follows the reference's adjoint conventions
 * (SURVEY.md App. B): Cholesky treated as constant, dH = -(LL^T)^-1 g_qdd * qdd^T accumulated over
 * the substeps that reuse a factor (matnn.h:310-336), min/max/clamp/step/normalize rules of
 * adjoint.h:129-190 and vec3.h:204-222.
 *
 * Defined on unit quaternions only, like the forward call whose checkpoint it consumes (precondition at dsim_step_forward).
 * QUATERNION COORDINATES, TWO FORMS.  For every quaternion block of joint_q (free joint: q[cs+3 .. cs+6], ball joint:
 * q[cs .. cs+3]) the reference's SimulateFunc.backward (sim.py:2127-2154) returns a cotangent WITH a component along the
 * quaternion itself: it differentiates its rotation formulas literally (quat.h:232-288 adj_mul / adj_rotate,
 * spatial.h:740-798), also in the direction in which |quat| changes, where those formulas are not rotations.  That "radial"
 * component is annihilated by the integrator's quaternion normalisation (sim.py:1552, 1616) in every upstream propagation --
 * gradients of rollouts w.r.t. actions do not depend on it -- and the adjoint kernels, where a pose cotangent is a world-frame
 * wrench, do not produce it:
 *   dsim_step_backward           gq_in == reference's gq_in minus, per quaternion block, (u . g_ref) u with u = quat / |quat|
 *                                (32 % / 16 % / 8 % of max |gq_in| on the Ant / Humanoid / SNUHumanoid recordings); every other
 *                                output (all non-quaternion coordinates of gq_in, gqd_in, gact, gmuscle_act) equals the
 *                                reference's to the fp32 tolerance.  The hot path: what DFlexEnv.step and SHAC use.
 *   dsim_step_backward_literal   gq_in == reference's gq_in, quaternion blocks included (measured against the reference's
 *                                recordings, UN-projected: 1.1e-6 / 5.8e-6 / 7.4e-6 max-norm relative, Ant / Humanoid /
 *                                SNUHumanoid).  The same adjoint launch + one small launch that evaluates the radial component
 *                                rho_j = dL/d eps_j under q_j -> (1 + eps_j) q_j in forward mode through the reference's literal
 *                                formulas of the first substep (csrc/dsim_literal.hpp) and adds rho_j q_j.  scratch:
 *                                [N][dsim_literal_scratch_floats(m)] floats of device memory the two launches hand over in
 *                                (the first substep's output cotangents and the first mass-matrix group's cotangent).
 *                                Models of up to 24 links / 28 dofs (DSIM_ERR_LIMIT beyond).
 * tests/test_gpu_parity.py asserts both statements on the HIP kernels' raw output. */
int dsim_step_backward(const dsim_model* m, int n_envs,
                       const float* ckpt, const float* act, const float* muscle_act,
                       float dt, int substeps, int mm_freq,
                       const float* gq_out, const float* gqd_out,
                       float* gq_in, float* gqd_in, float* gact, float* gmuscle_act, void* hip_stream);
int64_t dsim_literal_scratch_floats(const dsim_model* m);
int dsim_step_backward_literal(const dsim_model* m, int n_envs,
                               const float* ckpt, const float* act, const float* muscle_act,
                               float dt, int substeps, int mm_freq,
                               const float* gq_out, const float* gqd_out,
                               float* gq_in, float* gqd_in, float* gact, float* gmuscle_act, float* scratch, void* hip_stream);

/* Step Jacobians (ABI 110): many cotangents per environment from ONE checkpoint, in one launch of n_envs * n_cot workgroups
 * (workgroup e * n_cot + k: environment e, cotangent k; the plain one-environment-per-workgroup adjoint kernels).
 *
 * K cotangent pairs per environment against ONE checkpoint (read-only, shared by the K sweeps of an environment).
 * cot_shared != 0: gq_out [K][n_q], gqd_out [K][n_qd] are one set used by every environment;
 * cot_shared == 0: gq_out [N][K][n_q], gqd_out [N][K][n_qd].
 * Outputs WRITTEN: gq_in [N][K][n_q], gqd_in [N][K][n_qd], gact [N][K][n_qd] or NULL, gmuscle_act [N][K][M] or NULL.
 *
 * Both calls follow the conventions of dsim_step_backward above, row by row -- row (e, k) equals, bit for bit, what
 * dsim_step_backward returns for environment e with cotangent pair k:
 *   - the derivative is the one the adjoint defines: the factor treated as constant, dH accumulated over a mass-matrix group,
 *     the min / max / clamp rules of the reference;
 *   - the quaternion blocks of the q_in columns are TANGENT: they have no component along the quaternion (wrench form; there
 *     is no literal variant of these calls);
 *   - the checkpoint is consumed in the mode it was written in (DSIM_CKPT_FULL or DSIM_CKPT_LEAN), with the same act /
 *     muscle_act, dt, substeps and mm_freq as the forward call;
 *   - outputs are written, not accumulated; no host synchronisation, no atomics, the caller's stream;
 *   - n_cot <= 0 or a null required pointer (ckpt, act, muscle_act of a muscle model, gq_out, gqd_out, gq_in, gqd_in, J_state):
 *     DSIM_ERR_INVALID; n_envs * n_cot beyond the grid limit of 2^24 - 1 workgroups: DSIM_ERR_LIMIT, checked before anything
 *     is launched. */
int dsim_step_backward_multi(const dsim_model* m, int n_envs, int n_cot, int cot_shared,
                             const float* ckpt, const float* act, const float* muscle_act,
                             float dt, int substeps, int mm_freq,
                             const float* gq_out, const float* gqd_out,
                             float* gq_in, float* gqd_in, float* gact, float* gmuscle_act, void* hip_stream);
/* The whole Jacobian: row k is the gradient of output coordinate k of (q_out | qd_out), K = n_q + n_qd, seeded in the launch
 * (rows of an identity matrix the model holds on the device: n_cot = K, shared).
 * J_state [N][K][n_q + n_qd] (columns: q_in | qd_in), J_act [N][K][n_qd] or NULL, J_muscle [N][K][M] or NULL.
 * Rows and columns of a quaternion block: a COLUMN block (q_in) is tangent, as above -- J_state[e][k][block] . quat_in = 0; a ROW
 * of a quaternion output coordinate is the gradient of that coordinate of the renormalised quaternion, so the four rows of a
 * block are linearly dependent (quat_out^T rows = 0 to first order): A = J_state is the derivative in the redundant
 * coordinates, of rank n_q + n_qd minus the number of quaternion blocks. */
int dsim_step_jacobian(const dsim_model* m, int n_envs,
                       const float* ckpt, const float* act, const float* muscle_act,
                       float dt, int substeps, int mm_freq,
                       float* J_state, float* J_act, float* J_muscle, void* hip_stream);

/* Model parameters of the step, on the device (ABI 110: functions added).
 *
 * dsim_model_set_params overwrites ONE parameter array of the model's device-side constant block from DEVICE memory: a
 * device-to-device copy enqueued on hip_stream -- asynchronous, capturable in a HIP graph, no host synchronisation.
 *   field                          dev_values            (shapes of dsim_model_desc)
 *   DSIM_PARAM_TARGET_KE           [L]     joint_target_ke
 *   DSIM_PARAM_TARGET_KD           [L]     joint_target_kd
 *   DSIM_PARAM_LIMIT_KE            [L]     joint_limit_ke
 *   DSIM_PARAM_LIMIT_KD            [L]     joint_limit_kd
 *   DSIM_PARAM_TARGET              [n_q]   joint_target
 *   DSIM_PARAM_CONTACT_MATERIAL    [C][4]  contact_material (ke, kd, kf, mu per contact slot); C == 0: DSIM_OK, nothing done
 * ORDERING: the copy is ordered like a kernel of hip_stream.  Every launch on the model that is enqueued on that stream after
 * the call, or on a stream ordered after it (an event, a graph dependency), reads the new values -- the step kernels in every
 * launch mode, the fused env kernels, the read-outs, the literal launch; a launch that runs concurrently on an unordered
 * stream may read either.  The values are shared by all environments of the model and stay until the next call for that field
 * (nothing on the host is derived from these six arrays, so nothing else is recomputed).  dev_values may be reused once the
 * copy has run.  NULL dev_values or an unknown field: DSIM_ERR_INVALID. */
#define DSIM_PARAM_TARGET_KE 0
#define DSIM_PARAM_TARGET_KD 1
#define DSIM_PARAM_LIMIT_KE 2
#define DSIM_PARAM_LIMIT_KD 3
#define DSIM_PARAM_TARGET 4
#define DSIM_PARAM_CONTACT_MATERIAL 5
int dsim_model_set_params(dsim_model* m, int field, const float* dev_values, void* hip_stream);

/* Per-environment parameter VALUES (ABI 110: functions added): one constant block per environment instead of one for all.
 *
 * dsim_model_reserve_env_params with n_envs = R > 0 allocates a device block [R][W] -- W the model's whole constant block rounded
 * up to a multiple of 4 words, R * W * 4 bytes (W * 4: about 4.3 KB for Ant, 11.5 KB for Humanoid, 25.2 KB for SNUHumanoid) --,
 * re-allocating if R differs from what is reserved, fills EVERY row from the current shared block (what the model was created
 * with, or what dsim_model_set_params last wrote; a kernel on hip_stream) and switches the model to per-environment mode.  With
 * n_envs = 0 it frees the block and switches back to shared mode, under the shared block's values.  It allocates and frees
 * device memory, so it may synchronise the device, and it is NOT capturable: called while a capture is active on hip_stream it
 * changes nothing and returns DSIM_ERR_INVALID.  Reserve once, before capturing.
 * dsim_model_env_params returns R, or 0 in shared mode.
 *
 * In per-environment mode every launch on the model -- the step kernels in their plain and helper-wave launch modes, the fused
 * env kernels, the multi-cotangent and Jacobian launch, the parameter adjoint, the read-outs, the literal launch -- runs
 * environment e under row e: a launch of n_envs <= R environments uses the first n_envs rows, n_envs > R is DSIM_ERR_INVALID
 * (the message names both numbers; nothing is launched).  Environment e's results are BIT FOR BIT those of a shared-mode launch
 * under row e's values.  The two-environments-per-wavefront forward kernels share one copy of the constants between the two and
 * are not used in this mode: launches beyond the helper-wave capacity run the plain kernels.  dsim_step_backward_params then
 * returns per environment the gradient terms of THAT environment's values: do not sum them over the environments.
 *
 * dsim_model_set_env_params writes ONE parameter array of rows 0 .. n_envs - 1 from DEVICE memory: dev_values is
 * [n_envs][n] with the field's n as in the table above, 1 <= n_envs <= R.  One kernel launch on hip_stream -- asynchronous,
 * capturable, no host synchronisation -- with the ORDERING statement of dsim_model_set_params; rows from n_envs on keep their
 * values.  The contact field of a model with C == 0: DSIM_OK, nothing done.  DSIM_ERR_INVALID: NULL dev_values, an unknown
 * field, a model in shared mode, n_envs outside 1 .. R.
 * dsim_model_set_params keeps its meaning, "for ALL environments": in per-environment mode it writes the shared block as above
 * and broadcasts the array into every reserved row (one more launch on hip_stream, same ordering). */
int dsim_model_reserve_env_params(dsim_model* m, int n_envs, void* hip_stream);
int dsim_model_env_params(const dsim_model* m);
int dsim_model_set_env_params(dsim_model* m, int field, int n_envs, const float* dev_values, void* hip_stream);

/* dsim_step_backward with the gradients of those parameters: same arguments, same conventions, and gq_in, gqd_in, gact,
 * gmuscle_act equal to dsim_step_backward's BIT FOR BIT (the same arithmetic; one kernel family more, plain launch mode).
 * Two more outputs, both WRITTEN (not accumulated), either may be NULL but not both (DSIM_ERR_INVALID):
 *   g_dof     [N][5][n_qd]  per environment and dof, that dof's contribution to the gradient of (target_ke, target_kd, target,
 *                           limit_ke, limit_kd), summed over the substeps.  Kept per DOF: the caller folds dofs into links
 *                           (joint_qd_start; a ball joint's three dofs share one gain) or, for `target`, into the coordinate
 *                           of a hinge / slider dof, and sums over the environments -- the kernel sums neither (no atomics,
 *                           the same bits in every run).  With at the cotangent of the dof's tau in a substep (jcalc_tau,
 *                           sim.py:1452-1489):
 *                             revolute / prismatic   -(q - target) at, -qd at, +target_ke at, (lower - q) at or (upper - q) at
 *                                                    where the forward pass took that limit branch (else 0), -qd at (the limit
 *                                                    damping is unconditional);
 *                             ball                   -q[cs + k] at, -qd at, 0, 0, 0;   free / fixed: zeros.
 *   g_contact [N][C][4]     per environment and contact slot, the gradient of that contact's (ke, kd, kf, mu), summed over the
 *                           substeps (eval_rigid_contacts_art, sim.py:1137-1206): zeros for a contact that does not penetrate;
 *                           kf only in the kf |vt| < -mu c ke friction branch, mu only in the other.  Not touched when C == 0.
 * The checkpoint is consumed in the mode it was written in AND under the parameter values the forward call ran with: set the
 * same values again (dsim_model_set_params) if they were changed in between.  There is no literal or multi-cotangent variant of
 * this call; the fused env step has dsim_env_step_backward_params below. */
int dsim_step_backward_params(const dsim_model* m, int n_envs,
                              const float* ckpt, const float* act, const float* muscle_act,
                              float dt, int substeps, int mm_freq,
                              const float* gq_out, const float* gqd_out,
                              float* gq_in, float* gqd_in, float* gact, float* gmuscle_act,
                              float* g_dof, float* g_contact, void* hip_stream);

/* Derived body transforms of a joint state: X_sc[N][L][7] (link frames in the world, what eval_rigid_fk writes to
 * State.body_X_sc, sim.py:1638-1678) and, if X_sm is not NULL, X_sm[N][L][7] = X_sc o X_cm (State.body_X_sm: the bodies'
 * centre-of-mass frames).  The reference's State carries them after every forward() (model.py:338-392; read by
 * envs/snu_humanoid.py:209,227 for rendering) -- computed from the joint coordinates ENTERING the last substep; the
 * step functions above keep them in LDS / the checkpoint only, so this is the read-back: pass the q of interest (for the
 * reference's literal value: the head of the last substep's checkpoint row, which is that substep's input q). */
int dsim_body_transforms(const dsim_model* m, int n_envs, const float* q, float* X_sc, float* X_sm, void* hip_stream);

/* Differentiable body kinematics: link poses and twists of a given joint state, and the reverse pass.
 *   X_sc [N][L][7], X_sm [N][L][7]   as above, OF THE q HANDED IN (not the reference's one-substep lag, which stays a property
 *                                    of the State tensors the integrator returns);
 *   v_s  [N][L][6]                   world-frame spatial twist (w, v) of every link about the WORLD ORIGIN -- the reference's
 *                                    State.body_v_s (sim.py:1716-1789): the velocity of a point p of the link is v + w x p.
 * qd may be NULL: poses only, and v_s must be NULL too (v_s is returned if and only if qd is given); X_sm may be NULL.
 * The backward call maps cotangents on the three tensors (each may be NULL = zeros) to cotangents on q and qd, which are
 * WRITTEN, not accumulated (gqd is returned if and only if qd is given; gv_s needs qd).  It re-runs the kinematics on (q, qd):
 * nothing is kept between the two calls.  Pose cotangents are treated as world-frame wrenches, so, as
 * for the step adjoint above, the quaternion blocks of gq have NO component along the quaternion -- project the reference's
 * literal gradient onto the tangent space before comparing.
 * Like every call here: device pointers borrowed for the call, launches on the caller's stream, no host synchronisation,
 * deterministic (no atomics).  Precondition: unit quaternions in q; the forward call checks it like the step functions do (the
 * NEXT call on the model returns DSIM_ERR_INVALID), the backward call does not check again. */
int dsim_body_kinematics(const dsim_model* m, int n_envs, const float* q, const float* qd /* may be NULL */,
                         float* X_sc, float* X_sm /* may be NULL */, float* v_s /* NULL iff qd is NULL */, void* hip_stream);
int dsim_body_kinematics_backward(const dsim_model* m, int n_envs, const float* q, const float* qd /* may be NULL */,
                                  const float* gX_sc, const float* gX_sm, const float* gv_s /* each may be NULL = zeros */,
                                  float* gq, float* gqd /* NULL iff qd is NULL */, void* hip_stream);

/* Differentiable joint dynamics: generalized forces, accelerations and link forces of a given state, and the reverse pass.
 *   tau [N][nd]     the generalized force applied (the reference's State.joint_tau): -S . f_tot plus PD target, joint limits
 *                   and actuation;
 *   qdd [N][nd]     H(q)^-1 tau, the mass matrix ALWAYS built from the q handed in (State.joint_qdd of a refresh substep);
 *   f_s [N][L][6]   every link's OWN world-frame spatial force (torque about the world origin, force), the reference's
 *                   State.body_f_s: inertial force minus gravity, plus the ground contacts and muscles acting on the link.
 * One pass of the forward phases of a substep up to the solve: nothing is integrated, so there is no step length.  act and
 * muscle_act may be NULL (= zeros); each output may be NULL (skipped), not all three.
 * The backward call maps cotangents on the three tensors (each may be NULL = zeros) to cotangents on q, qd, act and muscle_act,
 * which are WRITTEN, not accumulated (gact and gmuscle_act may be NULL).  It re-runs the forward pass on (q, qd, act,
 * muscle_act): nothing is kept between the two calls.  Adjoint steps: adj qdd = gqdd; adj tau = H^-1 adj qdd + gtau; the
 * mass-matrix cotangent in the convention of the refresh substep above, dH = -(L L^T)^-1 g_qdd qdd^T (for one solve the exact
 * derivative); the per-dof adjoint of tau; gf_s added to the cotangent of the link's own force; then the mass-matrix and body
 * levels of the step adjoint.  Pose cotangents are world-frame wrenches: the quaternion blocks of gq have
 * NO component along the quaternion -- project the reference's literal gradient onto the tangent space before comparing.
 * Like every call here: device pointers borrowed for the call, launches on the caller's stream, no host synchronisation,
 * deterministic (no atomics).  Precondition: unit quaternions in q; the forward call checks it like the step functions do (the
 * NEXT call on the model returns DSIM_ERR_INVALID), the backward call does not check again. */
int dsim_joint_dynamics(const dsim_model* m, int n_envs, const float* q, const float* qd,
                        const float* act /* NULL = zeros */, const float* muscle_act /* NULL = zeros */,
                        float* tau, float* qdd, float* f_s /* each may be NULL, not all three */, void* hip_stream);
int dsim_joint_dynamics_backward(const dsim_model* m, int n_envs, const float* q, const float* qd,
                                 const float* act, const float* muscle_act,
                                 const float* gtau, const float* gqdd, const float* gf_s /* each may be NULL = zeros */,
                                 float* gq, float* gqd, float* gact /* may be NULL */, float* gmuscle_act /* may be NULL */,
                                 void* hip_stream);

/* Differentiable ground contacts: what the ground does to the robot in a given state, and the reverse pass.  C is the number
 * of contacts per environment, in model order (dsim_model_desc: contact_body / contact_point / contact_dist / contact_material).
 *   point [N][C][3]        the point tested against the ground: X_sc(body) o contact_point - n contact_dist with n = +y, so
 *                          point.y is the signed depth (negative = penetrating);
 *   vel [N][C][3]          v + w x point of the body's twist (the reference's dpdt);
 *   force [N][C][3]        normal + damping + friction force on the point (the reference's f_total, sim.py:1137-1206), EXACTLY zero
 *                          where point.y >= 0, with the roundings of the step kernels (their 1 / |vt|; zero friction at vt = 0);
 *   link_wrench [N][L][6]  per link the sum, in contact order, of (point x force, force): the contact part of State.body_f_s
 *                          (torque about the world origin, then force).
 * q and qd are both required; each output may be NULL (skipped), not all four.  A model without contacts succeeds: link_wrench is
 * zeros and the [N][0][3] outputs are not touched.
 * The backward call maps cotangents on the four tensors (each may be NULL = zeros) to cotangents on q and qd, which are WRITTEN,
 * not accumulated.  It re-runs the forward pass on (q, qd): nothing is kept between the two calls.  Per contact the derivative of
 * the force is the one the step adjoint uses: nothing where point.y >= 0 (an inactive contact contributes nothing through gforce
 * or glink_wrench), the damping term only where the normal velocity vn < 0, the friction magnitude by the branch
 * kf |vt| < mu |fn| as evaluated, and zero gradient of normalize and length at vt = 0.  gpoint and gvel are smooth and always
 * active.  Pose cotangents are world-frame wrenches: the quaternion blocks of gq have NO component along
 * the quaternion -- project the reference's literal gradient onto the tangent space before comparing.
 * Like every call here: device pointers borrowed for the call, launches on the caller's stream, no host synchronisation,
 * deterministic (no atomics).  Precondition: unit quaternions in q; the forward call checks it like the step functions do (the
 * NEXT call on the model returns DSIM_ERR_INVALID), the backward call does not check again. */
int dsim_ground_contacts(const dsim_model* m, int n_envs, const float* q, const float* qd,
                         float* point, float* vel, float* force, float* link_wrench /* each may be NULL, not all four */,
                         void* hip_stream);
int dsim_ground_contacts_backward(const dsim_model* m, int n_envs, const float* q, const float* qd,
                                  const float* gpoint, const float* gvel, const float* gforce,
                                  const float* glink_wrench /* each may be NULL = zeros */,
                                  float* gq, float* gqd, void* hip_stream);

/* Differentiable mass matrix: the joint-space inertia of a given q, its inverse and the joint motion axes, and the reverse pass.
 *   H [N][nd][nd]     the matrix the step inverts at a refresh substep of q: J^T M J (composite-rigid-body form) PLUS the joint
 *                     armature on the diagonal.  The reference's model.H is WITHOUT the armature (it adds it inside its
 *                     factorisation): model.H = H - diag(joint_armature);
 *   Hinv [N][nd][nd]  the Gauss-Jordan inverse of H exactly as the step kernels compute it: the same bits as the inverse a refresh
 *                     substep and dsim_joint_dynamics use for this q;
 *   S [N][nd][6]      the world-frame motion axis (angular, linear about the world origin) of every dof, the reference's
 *                     State.joint_S_s; the identity rows of a free joint are written too.  The Jacobian of link i is made of the
 *                     rows S_d of the dofs d of link i and its ancestors.
 * There is no qd and no step length: nothing here depends on them.  Each output may be NULL (skipped; without Hinv the inversion
 * is skipped as well), not all three.
 * The backward call maps cotangents on the three tensors (each may be NULL = zeros; gH and gHinv need not be symmetric) to the
 * cotangent on q, which is WRITTEN, not accumulated.  It re-runs the forward pass on q: nothing is kept between the two calls.
 * adj H = gH - Hinv^T gHinv Hinv^T with the kernel's own fp32 inverse, adj S = gS, then the mass-matrix and body levels of the
 * step adjoint.  Pose cotangents are world-frame wrenches: the quaternion blocks of gq have NO component
 * along the quaternion -- project the reference's literal gradient onto the tangent space before comparing.
 * Like every call here: device pointers borrowed for the call, launches on the caller's stream, no host synchronisation,
 * deterministic (no atomics).  Precondition: unit quaternions in q; the forward call checks it like the step functions do (the
 * NEXT call on the model returns DSIM_ERR_INVALID), the backward call does not check again. */
int dsim_mass_matrix(const dsim_model* m, int n_envs, const float* q,
                     float* H, float* Hinv, float* S /* each may be NULL, not all three */, void* hip_stream);
int dsim_mass_matrix_backward(const dsim_model* m, int n_envs, const float* q,
                              const float* gH, const float* gHinv, const float* gS /* each may be NULL = zeros */,
                              float* gq, void* hip_stream);

/* ---- fused environment surface -------------------------------------
 * The per-step torch glue of the reference environments -- action clip + scale into joint_act /
 * muscle activations (envs/ant.py:157-163, humanoid.py:188-211, snu_humanoid.py:245-271,
 * cartpole_swing_up.py:115-120), calculateObservations and calculateReward (ant.py:266-303,
 * humanoid.py:314-354, snu_humanoid.py:376-414, cartpole_swing_up.py:204-222) -- evaluated inside the
 * step kernels, adjoint included, so that one env.step() is ONE launch forward and ONE backward. */
#define DSIM_ENV_LOCOMOTION 1 /* free root: [h, quat(4), lin vel(3), ang vel(3), q[7:], s*qd[6:], up, heading, (actions)] */
#define DSIM_ENV_CARTPOLE 2   /* [x, xdot, sin th, cos th, thdot] */
#define DSIM_ENV_PLANAR 3     /* planar root (hopper, half-cheetah; envs/hopper.py:273, cheetah.py:254): [q[1:], qd] */
#define DSIM_REW_ANT 0
#define DSIM_REW_HUMANOID 1
#define DSIM_REW_SNU 2
#define DSIM_REW_CARTPOLE 3
#define DSIM_REW_HOPPER 4     /* cartpole_penalties[0] carries the termination angle */
#define DSIM_REW_CHEETAH 5

typedef struct dsim_env_spec {
    int32_t kind, rew_kind;
    int32_t n_act, n_obs;
    int32_t act_offset;   /* joint_act[act_offset + k] = clip(a_k,-1,1) * act_scale[k]        (act_muscle == 0) */
    int32_t act_muscle;   /* muscle_act[k] = (clip(a_k,-1,1) * 0.5 + 0.5) * act_scale[k]      (act_muscle == 1) */
    int32_t obs_actions;  /* observation ends with the stored actions */
    int32_t sanitize_grads; /* dsim_env_step_backward writes 0 for every non-finite cotangent it would return (gq_in, gqd_in,
                             * gactions): the nan_to_num(grad, 0, 0, 0) hooks that the reference's humanoid environments register on
                             * state.joint_q / joint_qd / actions in every step (envs/humanoid.py:195-206, snu_humanoid.py:253-264),
                             * done in the adjoint launch's own output stores instead of three extra torch kernels per step (ABI 106) */
    float inv_start_rot[4];
    float target_x, target_z;      /* targets + start_pos */
    float termination_height, termination_tolerance, height_rew_scale, action_penalty, joint_vel_obs_scaling;
    float cartpole_penalties[4];   /* pole angle, pole velocity, cart position, cart velocity */
    const float* act_scale;        /* [n_act] DEVICE pointer, borrowed per call */
} dsim_env_spec;

/* Episode bookkeeping fused into the step kernel.  Replaces, per env.step(), the torch ops and the device->host sync of
 * the reference: progress_buf += 1 and reset_buf at the end of calculateReward (envs/ant.py:176-184, 297-307;
 * humanoid.py:340-356; hopper.py:288-293), env_ids = reset_buf.nonzero() and reset(env_ids) (ant.py:186-234).
 * A finished environment e restarts from entry (reset_count[e] % reset_pool) of a pool of start states [normally one:
 * the deterministic start state], perturbed IN THE KERNEL when noise_q / noise_qd are given -- a fresh draw for every
 * restart, as the reference's reset() does with torch.rand (envs/ant.py:199-234, hopper.py:180-212,
 * cartpole_swing_up.py:140-160): coordinate k gets  + noise[k] * (u - 0.5)  with u uniform in [0, 1) from the counter-based
 * generator Philox4x32-10 keyed by `seed` at counter (environment index, reset_count[e], coordinate), so a restart never
 * repeats a state, needs no host work and is replay-safe under a captured HIP graph; for a free-floating root
 * (DSIM_ENV_LOCOMOTION) the start rotation is composed with a rotation by (u - 0.5) * noise_angle about a uniformly drawn
 * axis (normalize(u3 - 0.5), ant.py:208-213) and noise_q[3..6] is ignored.
 * q_out / qd_out / obs then describe the NEW state (stored actions cleared), obs_before_reset the old one, rew the old
 * one (0 for an invalid state), progress[e] = 0, done[e] = 1. */
typedef struct dsim_episode {
    int64_t* progress;          /* [N] in/out: progress_buf */
    int64_t* done;              /* [N] out: reset_buf */
    float* obs_before_reset;    /* [N][n_obs] out, may be NULL */
    const float* reset_q;       /* [reset_pool][N][n_q] */
    const float* reset_qd;      /* [reset_pool][N][n_qd] */
    int32_t* reset_count;       /* [N] in/out: restarts so far */
    int32_t reset_pool;
    int32_t episode_length;     /* done when progress > episode_length - 1 */
    int32_t height_terminate;   /* done when obs[0] < spec.termination_height */
    int32_t check_invalid;      /* done, reward 0, when obs / q / qd is non-finite or |q|, |qd| > 1e6 */
    const float* noise_q;       /* [n_q] DEVICE pointer or NULL: amplitude of the uniform restart noise per coordinate */
    const float* noise_qd;      /* [n_qd] DEVICE pointer or NULL */
    float noise_angle;          /* free-floating root: amplitude of the random start rotation (radians) */
    uint64_t seed;              /* Philox key */
} dsim_episode;

/* actions[N][n_act] -> q_out, qd_out, obs[N][n_obs], rew[N]  (+ ckpt as in dsim_step_forward; use dsim_ckpt_floats_mm).
 * episode may be NULL: plain step, no bookkeeping.  Same precondition and enforcement as dsim_step_forward: q_in holds
 * unit quaternions (the states this function returns, restarts included, always do). */
int dsim_env_step_forward(const dsim_model* m, const dsim_env_spec* env, int n_envs,
                          const float* q_in, const float* qd_in, const float* actions,
                          float dt, int substeps, int mm_freq,
                          float* q_out, float* qd_out, float* obs, float* rew, float* ckpt,
                          const dsim_episode* episode, void* hip_stream);

/* cotangents (gq_out, gqd_out, gobs, grew, gobs_before_reset) -> (gq_in, gqd_in, gactions).  Any of the five inputs may
 * be NULL (= zeros).  For an environment the forward step restarted, gq_out / gqd_out / gobs refer to the new state and
 * are ignored, as autograd does in the reference after reset()'s in-place writes. */
int dsim_env_step_backward(const dsim_model* m, const dsim_env_spec* env, int n_envs,
                           const float* ckpt, const float* actions,
                           float dt, int substeps, int mm_freq,
                           const float* gq_out, const float* gqd_out, const float* gobs, const float* grew,
                           const float* gobs_before_reset,
                           float* gq_in, float* gqd_in, float* gactions, void* hip_stream);

/* dsim_env_step_backward with the parameter gradients of dsim_step_backward_params: the same arguments in the same order, then
 * g_dof [N][5][n_qd] and g_contact [N][C][4] with the layout and the per-item terms documented there -- summed over the substeps
 * of this step, per environment, WRITTEN (callers may hand in uninitialised buffers), no atomics.  Either may be NULL; with both
 * NULL the call is the fused adjoint in the plain launch mode.  gq_in, gqd_in and gactions equal dsim_env_step_backward's BIT FOR
 * BIT (one kernel family more, one environment per workgroup, plain launch mode only).
 *   - The cotangents of the reward, the observation and obs_before_reset reach the parameters through the state they are
 *     functions of, so an environment the forward step restarted keeps the parameter terms of its reward and obs_before_reset
 *     cotangents (gq_out / gqd_out / gobs are ignored for it, as above).
 *   - An environment whose step ended invalid (the case in which dsim_env_step_backward returns zeros) gets zero rows.
 *   - With sanitize_grads set, g_dof and g_contact go through the same scrub as the three state cotangents.  A DELIBERATE
 *     EXTENSION: the reference's nan_to_num hooks sit on joint_q / joint_qd / actions only and do not cover model tensors, where
 *     one NaN would poison the parameter gradient of the whole rollout.
 * Same LDS limit (DSIM_ERR_LIMIT with the accumulators counted) and the same rule on parameter values as
 * dsim_step_backward_params: the checkpoint is consumed under the values the forward call ran with; in per-environment mode
 * n_envs may not exceed the reserved rows.  Capturable, no host synchronisation. */
int dsim_env_step_backward_params(const dsim_model* m, const dsim_env_spec* env, int n_envs,
                                  const float* ckpt, const float* actions,
                                  float dt, int substeps, int mm_freq,
                                  const float* gq_out, const float* gqd_out, const float* gobs, const float* grew,
                                  const float* gobs_before_reset,
                                  float* gq_in, float* gqd_in, float* gactions,
                                  float* g_dof, float* g_contact, void* hip_stream);

/* observation + reward of a given state with given stored actions (reset / initialize_trajectory path) */
int dsim_env_observe(const dsim_model* m, const dsim_env_spec* env, int n_envs, const float* q, const float* qd,
                     const float* stored_actions, float* obs, float* rew, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* DSIM_H */
