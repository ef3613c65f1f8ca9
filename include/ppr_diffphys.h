/*
 * ppr_diffphys.h -- C ABI of libpprdiffphys_hip.so (gfx950 / MI355X).
 *
 * This is the drop-in boundary for the ONE hot path of gengshan-y/ppr-diffphys:
 * the batched semi-implicit-Euler rigid-body rollout, its reverse-mode adjoint,
 * and forward kinematics.  Plain pointers and sizes only; every `float*` /
 * `int*` argument named *_dev is DEVICE memory (HBM) owned by the caller
 * (in the Python host: torch tensors), `stream` is a hipStream_t passed as void*.
 * All functions return 0 on success, non-zero on error (pd_last_error() has the text).
 * Nothing here allocates, frees or synchronises in the launch path (graph-capturable);
 * only pd_model_create / pd_model_destroy touch the allocator.
 *
 * What each entry point replaces in the reference (file:line under /root/reference):
 *
 *   pd_model_create      wp.sim.ModelBuilder.finalize + Model.collide
 *                        (diffphys/dp_model.py:384-401; arrays per SURVEY.md App. A.2)
 *   pd_rollout_forward   ForwardWarp.forward (diffphys/dp_model.py:1146-1249): eval_fk, then per step
 *                        clear_forces + wp_add (:1210-1221) + SemiImplicitIntegrator.simulate
 *                        (diffphys/integrator_euler.py:579-620: eval_body_contacts :93-179,
 *                        eval_body_joints :289-451, integrate_bodies :21-91), frame gather (:1241-1248)
 *   pd_rollout_backward  ForwardWarp.backward (diffphys/dp_model.py:1251-1400): wp.Tape.backward over the
 *                        same launches, gradients of the 11 inputs
 *   pd_fk_forward/backward  ForwardKinematics.forward/backward (diffphys/dp_model.py:1022-1130),
 *                        i.e. warp.sim.articulation.eval_fk and its tape adjoint
 *
 * Layouts are the reference's flat env-major ones:
 *   q_init [bs*nq]   qd_init [bs*nqd] (root twist as (w, v))
 *   torques, refs [T][bs*nqd]         res_f [T][bs*nb][6] (tau, f)
 *   target_ke, target_kd [bs*nqd]     body_mass, body_inv_mass [bs*nb]
 *   body_inertia, body_inv_inertia [bs*nb][3][3] row-major
 *   wp_pos [F][bs*nb][7] (p, q=xyzw)  wp_vel [F][bs*nb][6] (w, v)   grf, jaf [F][bs*nb][6]
 * The saved trajectory (workspace) is internal SoA: see pd_rollout_workspace_floats.
 */
#ifndef PPR_DIFFPHYS_H
#define PPR_DIFFPHYS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PD_ABI_VERSION 9   /* 2: host frame2step (validated), per-model timing, per-env joint_X_p binding; 3: pose algebra + foot height; 4: gradient post-processing (remove_nan / FK clamp) inside the kernels, pd_build_id; 5: pd_model_contact_order (decoding the hit log), pd_rollout_forward_traj_loss / pd_rollout_backward_traj_loss (row f4), pd_model_set_kernel_family (quad-lane small-batch kernels); 6: pd_rollout_forward_traj_loss_fk / pd_rollout_backward_traj_loss_fk (the FK of the control reference rides on the trajectory-loss launches); 7: pd_reduce_loss (reduce_loss on any table, threshold from env 0 as the reference takes it), pd_model_set_numeric_policy (the reference's literal acos forms as a run-time mode); 8: pd_colsum; 9: pd_linear_wgrad (the time-MLPs' weight + bias gradients on the fp32 matrix cores) */

/* Articulation template: HOST pointers, copied by pd_model_create.  One template for all envs. */
typedef struct pd_model_desc {
  int nb, nq, nqd;              /* bodies (= joints), joint coords, joint dofs per env */
  int nc, nmat;                 /* ground-contact candidate points, materials */
  const int *joint_type;        /* [nb] Warp codes: 1 revolute, 3 fixed, 4 free, 5 compound */
  const int *joint_parent;      /* [nb] -1 for the root; parents precede children */
  const int *joint_q_start;     /* [nb] */
  const int *joint_qd_start;    /* [nb] */
  const float *joint_X_p;       /* [nb][7] parent-frame joint transform (p, q) */
  const float *joint_X_c;       /* [nb][7] child-frame joint transform */
  const float *joint_axis;      /* [nb][3] */
  const float *body_com;        /* [nb][3] */
  const float *joint_limit_lower, *joint_limit_upper, *joint_limit_ke, *joint_limit_kd; /* [nqd] */
  const int *contact_body;      /* [nc] body index of each candidate point */
  const float *contact_point;   /* [nc][3] body frame */
  const float *contact_dist;    /* [nc] shape thickness */
  const int *contact_material;  /* [nc] index into shape_materials */
  const float *shape_materials; /* [nmat][4] (ke, kd, kf, mu) */
  float gravity[3];
  float joint_attach_ke, joint_attach_kd;
} pd_model_desc;

typedef struct pd_model pd_model; /* opaque; owns the device copy of the template */

int pd_abi_version(void);
/* "<git HEAD at build time>+<first 16 hex digits of the sha256 over the library's sources>" (csrc/Makefile: SRCS, in that order).
 * A loader that also has the sources (tests, __graft_entry__.smoke) compares the hash: a stale binary cannot pass for the tree's. */
const char *pd_build_id(void);
const char *pd_last_error(void);

/* Placement of the contact tables (up to 65 535 candidates): the rollout kernels copy them into LDS once per workgroup, beside the
 * envs' scratch, and the default segment width is the narrowest >= nb at which both fit 160 KiB.  A robot whose tables fit at NO
 * width (more than ~7 000 mesh candidates) keeps them in global memory instead: then the default is the narrowest width at which
 * its envs' scratch alone fits, and only a robot whose scratch fits at no width is refused ("model needs N B of LDS ..."). */
int pd_model_create(const pd_model_desc *desc, pd_model **out);
void pd_model_destroy(pd_model *m);
/* Lanes of a 64-wide wavefront given to one articulation: 16, 32 or 64 (>= nb).  0 = default
 * (smallest that fits).  64 is the literal "one articulation per wavefront" mapping.  The tables stay where pd_model_create put
 * them: a model with tables in global memory accepts every width at which its envs' scratch fits. */
int pd_model_set_segment_width(pd_model *m, int lanes);
int pd_model_get_segment_width(const pd_model *m);

/* Kernel family of the rollout launches.  0 (default): chosen per launch by batch size -- revolute-only robots with at most 16 bodies
 * (Laikago) run the QUAD-LANE kernels (four lanes per body, one articulation per wavefront: a shorter instruction stream per step,
 * three times the lane-cycles per env) while the batch fits one workgroup per compute unit (<= 4 x CUs envs = 1 024 on MI355X) and the
 * lane-per-body kernels above that; 1: lane per body always; 2: quad-lane wherever the robot is eligible (tests, A/B timing).
 * pd_model_get_kernel_family returns the setting; *eligible (may be NULL) = 1 when the robot has quad-lane kernels at all (whether
 * its contact tables live in LDS or, when they fit at no segment width, in global memory).
 *
 * Parent-side joint frames (tests, A/B timing; no new entry: the choice rides on `family`).  A revolute-only robot whose joint_X_p
 * rotations are all bitwise (0, 0, 0, 1) -- Laikago -- qualifies for lane-per-body adjoint kernels compiled without the product
 * q_p = q_parent (x) q_pj and its adjoint; by default such a robot's adjoint launches take them (not while a per-env joint_X_p is bound:
 * device data the host has not seen).  family + PD_PFI_GENERAL: the general kernels always; family + PD_PFI_SPECIALISED: refused with an
 * error unless the robot qualifies; a plain 0 .. 2 is automatic again.  pd_model_get_kernel_family returns what was set, sum included.
 * pd_last_launch_info(m, PD_LAUNCH_INFO_PARENT_FRAMES, out) tells whether the robot qualifies and what the last adjoint launch ran.
 *
 * Model facts.  A qualifying robot that also has no joint limit gains (joint_limit_ke = joint_limit_kd = 0 for the dof of every revolute joint), a FREE root joint
 * with at least six bodies behind it and no body with more than four children -- Laikago -- takes, by default, the same kernels with these
 * facts compiled in instead of tested in every step.  + PD_PFI_NO_FACTS (on top of any of the above): keep the kernels that test them.
 * PD_PFI_GENERAL still forces the fully general kernels.
 *
 * Com facts.  A robot with its model facts compiled in whose centres of mass (body_com, as fp32) all have x == 0 and y == 0, and are
 * (0, 0, 0) for every body whose joint is not FREE -- Laikago again -- takes, by default, kernels that also leave out the products with those
 * zeros.  + PD_PFI_NO_COM_FACTS: keep the kernels with the general centre-of-mass algebra.  (A non-finite state no longer meets 0 * x there.) */
#define PD_PFI_GENERAL 4
#define PD_PFI_SPECIALISED 8
#define PD_PFI_NO_FACTS 16
#define PD_PFI_NO_COM_FACTS 32
int pd_model_set_kernel_family(pd_model *m, int family);
int pd_model_get_kernel_family(const pd_model *m, int *eligible);

/* Numeric policy of the rollout launches of this model (ABI v7) -- HOW two expressions of the joint pass are evaluated in fp32, forward
 * and adjoint, both kernel families; the functions are the same, a float64 evaluation of either policy gives the same numbers:
 *   PD_NUM_STABLE  (default)  revolute twist angle q = 2 sign(d) atan2(|axis| |d|, r.w), d = r.xyz . axis; FIXED joint's angular error
 *                  r.xyz * 2 atan2(|r.xyz|, r.w) / |r.xyz| -- accurate to an ulp at joint angle 0 / at the joint's operating point
 *   PD_NUM_LITERAL the reference's text, diffphys/integrator_euler.py:385-400: twist = normalize((axis d, r.w)), q = 2 acos(twist.w)
 *                  sign(axis . twist.xyz); FIXED: normalize(r.xyz) * acos(r.w) * 2; adjoints through acos' (0 at |x| = 1, argument clamped
 *                  to [-1, 1]: the policy of both modes) and the normalisations.  In fp32 acos near 1 turns one ulp of twist.w into 7e-4
 *                  rad of a small joint angle: use it for a side-by-side run against the reference on Warp,
 *                  expect it 1e-3 .. 1 away from a float64 evaluation in long-horizon gradients where PD_NUM_STABLE is 1e-5 .. 1e-3.
 * May be changed between launches; a forward pass and its adjoint must run under the same policy. */
#define PD_NUM_STABLE 0
#define PD_NUM_LITERAL 1
int pd_model_set_numeric_policy(pd_model *m, int policy);
int pd_model_get_numeric_policy(const pd_model *m);

/* Floats of caller-provided workspace that pd_rollout_forward fills and pd_rollout_backward reads:
 * per step the 13-float body state and the 6-float body wrench as five float4 planes [step][plane][bs*nb], followed
 * by the forward sweep's contact hit log (32 ints per env-step) that the adjoint replays.  The base must be 16-byte
 * aligned.  A forward with no adjoint to follow needs none (NULL: forward-only, see pd_rollout_forward). */
size_t pd_rollout_workspace_floats(const pd_model *m, int bs, int nsteps);

/* Inspection of the saved trajectory (tests, diagnostics): the hit log behind the planes holds, per (step, env), 32 ints --
 * [0] the number n of contact candidates that touched in that step (eval_body_contacts' `c <= 0`, integrator_euler.py:130-133;
 * -1 when more than 31 did: the adjoint then sweeps again), [1..n] packed entries  point | material << 16 | body << 24  with
 * `point` an index into the DEVICE contact table (candidates grouped by body, spatially ordered inside a body).
 * order_host[i] (HOST, capacity >= nc ints) receives the index into the template's contact_* arrays of device entry i. */
int pd_model_contact_order(const pd_model *m, int *order_host, int capacity);

/* Per-env joint_X_p (the lab4d path rebinds env.joint_X_p from a torch tensor before every rollout,
 * diffphys/dp_interface.py:465): joint_X_p_dev is [n_envs][nb][7] DEVICE memory owned by the caller and read by every
 * later launch on this model until it is re-bound; NULL / 0 returns to the template's joint_X_p.  A rollout then needs
 * bs == n_envs; FK articulation i uses env i % n_envs (the reference runs eval_fk frame by frame on the same n_envs
 * model).  Host-side pointer swap only: no copy, no synchronisation, no rebuild of the device model. */
int pd_model_bind_joint_X_p(pd_model *m, const float *joint_X_p_dev, int n_envs);

/* frame2step_host: [nframes] HOST ints, frame f is state frame2step[f] (ForwardWarp reads self.frame2step,
 * diffphys/dp_model.py:1231-1248).  Validated before anything is launched: each entry in 0..nsteps, no step twice
 * (a violation returns non-zero, nothing is written).  State `nsteps` (the state after the last step) is a legal frame
 * for wp_pos / wp_vel; its grf / jaf rows are zero -- the reference appends no force snapshot for it (:1225-1228).
 * The device-side step->frame table is cached per model and (nsteps, frame2step); the first call with a new key uploads
 * it with one synchronous copy, later calls neither allocate nor synchronise (warm up before capturing a graph).
 * Sizes: bs = 0 and nsteps = 0 are legal (nothing / FK only).  Largest batch of ONE call: bs x bodies < 2^27 and bs < 2^24 (the kernels
 * add 32-bit lane offsets to 64-bit step bases; 10 M Laikago envs) -- a larger bs is refused (non-zero, "batch too large"), never
 * wrapped; the workspace and every tensor may lie past 4 GiB (tests: 1 048 576 envs x 8 steps, 9.8 GB of workspace).
 * Forward-only: workspace_dev == NULL with nsteps > 0 is accepted (here and in the two *_traj_loss forward entries).  Such a launch
 * saves nothing for the adjoint -- no trajectory, no hit log, and on the loss entries no seeds: seed_pos_dev and seed_gt_dev must be
 * NULL too (a non-NULL one is refused with a message) -- and writes only wp_pos / wp_vel / grf / jaf, plus, on the loss entries,
 * loss_table / reduced / scale and the FK rows.  Those are bit-identical to a launch with a workspace.  No adjoint can follow it: the
 * pd_rollout_backward* entries refuse a NULL workspace.  (Laikago: 456 bytes of inputs per env-step instead of 1 624 with the
 * workspace.)  With nsteps == 0 there is no trajectory either way and NULL keeps meaning "no workspace needed".
 * Resumed: qd_init_dev == NULL (with bs > 0 and q_init_dev non-NULL) starts the rollout from a BODY state instead of joint
 * coordinates.  q_init_dev is then [bs*nb][13] = (p[3], q[4] xyzw, w[3], v[3]) per body: the body-origin pose and the twist, exactly
 * the numbers of a wp_pos row followed by a wp_vel row.  The 13 floats are used as they are -- no FK, the quaternion is not
 * re-normalised -- so the rows of an earlier rollout's frame at its state nsteps continue that rollout bit for bit; a frame at step
 * 0 returns the state bit for bit.  Frames, workspace or none, forces: as before.  pd_rollout_forward / pd_rollout_backward only: the
 * *_traj_loss entries refuse a NULL qd_init_dev with a message.  The adjoint of such a rollout: pd_rollout_backward with
 * qd_init_dev == NULL and the same state in q_init_dev; g_q_init_dev then receives the gradient of the body state, [bs*nb][13], and
 * g_qd_init_dev must be NULL (a non-NULL one is refused with a message, nothing is written).  That state gradient is stored RAW, without
 * the remove_nan every other gradient gets: it is the adjoint that flows on into the rollout that produced the state -- as the seed
 * (adj_pos / adj_vel rows) of that rollout's frame at its state nsteps -- and a single launch does not scrub it between steps either.
 * Zero controls: torques_dev and res_f_dev may each be NULL with nsteps > 0, alone or together, here and in the two *_traj_loss forward
 * entries.  NULL means "all zeros" -- what the reference feeds the rollout after multiplying both MLP outputs by zero
 * (diffphys/dp_model.py:526-536): nothing is read for that input and the caller allocates nothing for it (Laikago: 384 of the 456 bytes of
 * inputs per env-step).  Every output -- wp_pos / wp_vel / grf / jaf, the workspace with its hit log, and on the loss entries seeds, loss
 * table, reduced, scale and the FK rows -- is bit-identical to the launch that is given zero-filled tensors.  Such a launch runs a
 * zero-controls instantiation of the forward kernel (the loads of the two inputs behind wave-uniform tests of their pointers, an absent
 * one yielding 0.0f into the same arithmetic); with both given the kernel is the one it always was.  Composes with Forward-only
 * (NULL workspace) and Resumed (NULL qd_init_dev), both numeric policies, both kernel families, every segment width and both table
 * placements; neither allocates nor synchronises, so it may be captured.  refs_dev stays required with nsteps > 0 -- a PD target of zero
 * is a pose, not an absence: a NULL one is refused by name ("null device pointer: refs_dev ...") and nothing is written -- as does
 * every other input.  The adjoint of such a rollout: see pd_rollout_backward, Zero controls.
 * These argument combinations were refused ("null device pointer") before; no symbol or signature changed, the version stays 9. */
int pd_rollout_forward(const pd_model *m, int bs, int nsteps, float dt,
                       const float *q_init_dev, const float *qd_init_dev, const float *torques_dev,
                       const float *res_f_dev, const float *refs_dev, const float *target_ke_dev,
                       const float *target_kd_dev, const float *body_inv_mass_dev,
                       const float *body_inertia_dev, const float *body_inv_inertia_dev,
                       int nframes, const int *frame2step_host, float *workspace_dev,
                       float *wp_pos_dev, float *wp_vel_dev, float *grf_dev, float *jaf_dev, void *stream);

/* Gradients are OVERWRITTEN (not accumulated).  g_*_dev mirror the input shapes.  body_mass has no
 * direct gradient (integrator_euler.py:43 loads it, nothing uses it), so there is no g_body_mass.
 * Every stored gradient has been through the boundary's remove_nan (diffphys/dp_model.py:1294-1384 with
 * diffphys/dp_utils.py:43-57, clip=False): NaN -> 0, +-inf kept -- applied by the kernel at its stores (ABI v4; up to v3
 * the caller had to scrub).
 * Selective: each of g_torques_dev, g_res_f_dev and g_refs_dev -- the three gradients with a row PER STEP, [T][bs*nqd], [T][bs*nb][6],
 * [T][bs*nqd]: 456 bytes per Laikago env-step together -- may be NULL, here and in the two *_traj_loss backward entries, alone or in
 * any combination (all three NULL included).  NULL means "not wanted": the launch computes nothing for that gradient and stores
 * nothing for it, and the caller allocates nothing.  Every gradient that IS asked for -- the remaining per-step ones, g_q_init /
 * g_qd_init, the state gradient of a resumed rollout, the five summed ones, the FK ride's -- is bit-identical to what the launch with
 * all three pointers stores.  Such a launch runs a selective instantiation of the adjoint kernel (its per-step stores behind
 * wave-uniform tests of the pointers); with all three given the kernel is the one it always was.  Composes with Resumed
 * (qd_init_dev == NULL); neither allocates nor synchronises, so it may be captured.  The INPUT refs_dev and the
 * workspace stay required with nsteps > 0, and every other g_*_dev stays required.
 * Zero controls: torques_dev may be NULL with nsteps > 0 ("all zeros"), here and in the two *_traj_loss backward entries; res_f is not
 * an input of the adjoint.  CONTRACT: the adjoint's torques_dev is NULL exactly when the forward's was (or, equally, the forward was given
 * zeros).  A mismatch cannot be detected -- the workspace does not record it -- and is the caller's error, like a numeric-policy mismatch:
 * the gradients are then those of another rollout.  g_torques_dev and g_res_f_dev are independent of this: the gradient with respect to
 * an absent, zero input is well defined, it is computed when its pointer is given, and it equals the zero-tensor launch's bit for bit, as
 * does every other gradient.  A NULL torques_dev takes the selective instantiation too (the load behind a test of the pointer), whatever
 * the g_*_dev are; composes with Selective and Resumed.  A NULL refs_dev is refused by name, nothing is written.
 * These argument combinations were refused ("null device pointer") before; no symbol or signature changed, the version stays 9. */
int pd_rollout_backward(const pd_model *m, int bs, int nsteps, float dt,
                        const float *q_init_dev, const float *qd_init_dev, const float *torques_dev,
                        const float *refs_dev, const float *target_ke_dev, const float *target_kd_dev,
                        const float *body_inv_mass_dev, const float *body_inertia_dev,
                        const float *body_inv_inertia_dev, int nframes, const int *frame2step_host,
                        const float *workspace_dev, const float *adj_pos_dev, const float *adj_vel_dev,
                        float *g_q_init_dev, float *g_qd_init_dev, float *g_torques_dev, float *g_res_f_dev,
                        float *g_refs_dev, float *g_target_ke_dev, float *g_target_kd_dev,
                        float *g_body_inv_mass_dev, float *g_body_inertia_dev, float *g_body_inv_inertia_dev,
                        void *stream);

/* The rollout with the trajectory loss evaluated where the frame poses are produced.  Of the reference's
 * loss terms only loss_traj back-propagates through the rollout (diffphys/dp_model.py:777-779; pos_state / vel_state / distill use
 * sim_position.detach(), :795,802):   loss_traj = reduce_loss(se3_loss(sim_position, target_position).mean(-1) with outseq entries
 * zeroed, clip=True)   (se3_loss diffphys/dp_utils.py:113-138, reduce_loss :93-110).
 * pd_rollout_forward_traj_loss = pd_rollout_forward plus, inside the same rollout launch, at every frame state: se3_loss of each body
 * pose against target_pos_dev [bs][F][nb][7] (p, real-last quaternion), its UNSCALED gradients to seed_pos_dev [F][bs*nb][7] (the
 * layout of adj_pos) and seed_gt_dev [bs][F][nb][7] (d / d target; may be NULL), the mean over the env's bodies to
 * loss_table_dev [bs][F] (0 where outseq_dev [bs][F] bytes are non-zero; outseq_dev may be NULL); then one small launch that does
 * reduce_loss on the table: reduced_dev[4] = { loss_traj, the clip threshold (10 x the lower median of the positive entries of
 * ENV 0, as the reference takes it, dp_utils.py:98-100; NaN when env 0 has none, and then -- like the reference -- no env is
 * clipped), the number of positive entries left, the number of clipped envs } and scale_dev [bs][F] =
 * d loss_traj / d table entry (0 for entries the clip / outseq assigned zero).  wp_pos / wp_vel / grf / jaf as pd_rollout_forward.
 * pd_rollout_backward_traj_loss = pd_rollout_backward whose frame seeds are  g_loss_dev[0] * scale[env][frame] / nb * seed_pos
 * (g_loss_dev: DEVICE scalar, the upstream gradient of loss_traj, e.g. traj_wt) PLUS the rows of adj_pos_dev / adj_vel_dev when
 * those are given (both or neither; NULL = no other term reaches the poses); they are built by a small launch into
 * seed_work_dev (F * bs * nb * 13 floats of caller-owned scratch) in front of the adjoint rollout launch.  No pose or seed passes
 * through the host framework between the launches, no se3_loss launch, no reduce_loss ops. */
int pd_rollout_forward_traj_loss(const pd_model *m, int bs, int nsteps, float dt,
                                 const float *q_init_dev, const float *qd_init_dev, const float *torques_dev,
                                 const float *res_f_dev, const float *refs_dev, const float *target_ke_dev,
                                 const float *target_kd_dev, const float *body_inv_mass_dev,
                                 const float *body_inertia_dev, const float *body_inv_inertia_dev,
                                 int nframes, const int *frame2step_host, float *workspace_dev,
                                 float *wp_pos_dev, float *wp_vel_dev, float *grf_dev, float *jaf_dev,
                                 const float *target_pos_dev, const unsigned char *outseq_dev, float rot_ratio,
                                 float *seed_pos_dev, float *seed_gt_dev, float *loss_table_dev, float *reduced_dev,
                                 float *scale_dev, void *stream);
int pd_rollout_backward_traj_loss(const pd_model *m, int bs, int nsteps, float dt,
                                  const float *q_init_dev, const float *qd_init_dev, const float *torques_dev,
                                  const float *refs_dev, const float *target_ke_dev, const float *target_kd_dev,
                                  const float *body_inv_mass_dev, const float *body_inertia_dev,
                                  const float *body_inv_inertia_dev, int nframes, const int *frame2step_host,
                                  const float *workspace_dev, const float *adj_pos_dev, const float *adj_vel_dev,
                                  const float *seed_pos_dev, const float *scale_dev, const float *g_loss_dev,
                                  float *seed_work_dev, float *g_q_init_dev, float *g_qd_init_dev, float *g_torques_dev, float *g_res_f_dev,
                                  float *g_refs_dev, float *g_target_ke_dev, float *g_target_kd_dev,
                                  float *g_body_inv_mass_dev, float *g_body_inertia_dev, float *g_body_inv_inertia_dev,
                                  void *stream);

/* Row f4, second half: the FK of the control reference (ForwardKinematics.apply(queried_q, queried_qd, env), diffphys/dp_model.py:758
 * of the reference: F x bs chains per iteration, independent of the rollout) without a launch of its own.  The two entries below are
 * the *_traj_loss entries above with one more argument; with fk != NULL and fk->n > 0
 *   forward : the small launch that follows the rollout launch runs reduce_loss in its first workgroup and FK forward in the others;
 *   backward: the small launch in front of the adjoint rollout builds the seeds in its first workgroups and runs FK backward
 *             (with ForwardKinematics.backward's post-processing, see pd_fk_backward) in the others.
 * The articulations come FRAME-major, joint_q [F][bs][nq] / joint_qd [F][bs][nqd] (n = F * bs; F need not be the rollout's nframes) --
 * the layout of ForwardKinematics' rj_q / rj_qd -- and the body rows are ENV-major, [bs][F][nb][7] / [bs][F][nb][6] (what the
 * reference gets from permute(1, 0, 2, 3) at dp_model.py:1093-1094, and what its losses consume): no permuted copy on either side.
 * Forward reads joint_q / joint_qd, writes body_q / body_qd; backward reads joint_q / joint_qd / adj_body_q / adj_body_qd, writes
 * g_joint_q / g_joint_qd; the other fields may be NULL.  fk == NULL or fk->n == 0: exactly the *_traj_loss entries. */
typedef struct pd_fk_ride {
  int n, bs;
  const float *joint_q_dev, *joint_qd_dev;
  float *body_q_dev, *body_qd_dev;
  const float *adj_body_q_dev, *adj_body_qd_dev;
  float *g_joint_q_dev, *g_joint_qd_dev;
} pd_fk_ride;
int pd_rollout_forward_traj_loss_fk(const pd_model *m, int bs, int nsteps, float dt,
                                    const float *q_init_dev, const float *qd_init_dev, const float *torques_dev,
                                    const float *res_f_dev, const float *refs_dev, const float *target_ke_dev,
                                    const float *target_kd_dev, const float *body_inv_mass_dev,
                                    const float *body_inertia_dev, const float *body_inv_inertia_dev,
                                    int nframes, const int *frame2step_host, float *workspace_dev,
                                    float *wp_pos_dev, float *wp_vel_dev, float *grf_dev, float *jaf_dev,
                                    const float *target_pos_dev, const unsigned char *outseq_dev, float rot_ratio,
                                    float *seed_pos_dev, float *seed_gt_dev, float *loss_table_dev, float *reduced_dev,
                                    float *scale_dev, const pd_fk_ride *fk, void *stream);
int pd_rollout_backward_traj_loss_fk(const pd_model *m, int bs, int nsteps, float dt,
                                     const float *q_init_dev, const float *qd_init_dev, const float *torques_dev,
                                     const float *refs_dev, const float *target_ke_dev, const float *target_kd_dev,
                                     const float *body_inv_mass_dev, const float *body_inertia_dev,
                                     const float *body_inv_inertia_dev, int nframes, const int *frame2step_host,
                                     const float *workspace_dev, const float *adj_pos_dev, const float *adj_vel_dev,
                                     const float *seed_pos_dev, const float *scale_dev, const float *g_loss_dev,
                                     float *seed_work_dev, float *g_q_init_dev, float *g_qd_init_dev, float *g_torques_dev, float *g_res_f_dev,
                                     float *g_refs_dev, float *g_target_ke_dev, float *g_target_kd_dev,
                                     float *g_body_inv_mass_dev, float *g_body_inertia_dev, float *g_body_inv_inertia_dev,
                                     const pd_fk_ride *fk, void *stream);

/* n independent articulations: joint_q [n][nq], joint_qd [n][nqd] -> body_q [n][nb][7], body_qd [n][nb][6] */
int pd_fk_forward(const pd_model *m, int n, const float *joint_q_dev, const float *joint_qd_dev,
                  float *body_q_dev, float *body_qd_dev, void *stream);
/* The gradients come out with ForwardKinematics.backward's post-processing (diffphys/dp_model.py:1109-1110, 1122-1123):
 * NaN -> 0, then values above 1 -> 1 (an upper clamp only) -- applied by the kernel at its stores (ABI v4). */
int pd_fk_backward(const pd_model *m, int n, const float *joint_q_dev, const float *joint_qd_dev,
                   const float *adj_body_q_dev, const float *adj_body_qd_dev,
                   float *g_joint_q_dev, float *g_joint_qd_dev, void *stream);

/* Fused per-frame pose loss and its gradients (replaces the torch composition of
 * se3_loss, diffphys/dp_utils.py:113-138):  n elements of `dim` floats, dim = 7 (p, real-last quaternion) or 6
 * (p, axis-angle).  loss[n]; g_pred / g_gt [n][dim] = d loss / d input (either may be NULL).  Entries with a NaN input
 * give loss 0 and gradients 0 x (the raw gradient), i.e. NaN where the local derivative is not finite and 0 elsewhere -- what autograd
 * makes of the reference's `loss[nanid] = 0` (dp_utils.py:137): the NaN reaches the adjoint rollout as a seed there too and is scrubbed
 * at that boundary (remove_nan), which drops the env's whole gradient. */
int pd_se3_loss(int n, int dim, const float *pred_dev, const float *gt_dev, float rot_ratio, float *loss_dev,
                float *g_pred_dev, float *g_gt_dev, void *stream);

/* reduce_loss of the reference (diffphys/dp_utils.py:93-110) on any [bs][nframes] device table (ABI v7) -- the same one-workgroup code
 * the trajectory-loss entries run after the rollout, callable on its own (the reference also reduces its other loss terms with it,
 * dp_model.py:797-809, clip = 0 there).  clip != 0: the threshold is 10 x the lower median (torch.median) of env 0's positive entries,
 * taken once and used for every env; each env's entries from the first one above it on are ASSIGNED zero IN table_dev (the reference
 * truncates its argument in place); env 0 without a positive entry: the threshold is NaN and nothing is clipped (what the reference
 * does on torch >= 1.8: tests/golden/ref_host_reduce_loss.npz holds its outputs).  The value is the mean of the positive entries
 * left when the sum of all entries is positive, else the mean of all entries (NaN entries make that NaN, as in the reference).
 * reduced_dev[4] = { value, threshold, positive entries left, clipped envs }; scale_dev [bs][nframes] (may be NULL) = d value /
 * d entry (0 for assigned entries).  An empty table gives 0. */
int pd_reduce_loss(int bs, int nframes, float *table_dev, int clip, float *reduced_dev, float *scale_dev, void *stream);

/* SE(3) pose algebra of the loss plumbing, one launch per op and one per vector-Jacobian
 * product; replaces the reference's compositions of dqtorch kernels and torch ops:
 *   PD_POSE_COMPOSE_DELTA  a = target pose [n][7] (p, real-last quaternion), b = delta [n][6] (p, axis-angle) -> out [n][7]
 *                          = se3_mat2vec(se3_vec2mat(delta) @ se3_vec2mat(target))        diffphys/dp_utils.py:22-31
 *   PD_POSE_ROTATE_FRAME   a = global pose, b = target pose [n][7] -> out [n][7] = T_global @ T_target   dp_utils.py:60-73
 *   PD_POSE_ROTATE_VEL     a = global pose, b = (linear, angular) [n][6] -> out [n][6], both halves rotated by the
 *                          rotation of the global pose                                    dp_utils.py:76-84
 * with se3_vec2mat / se3_mat2vec / quaternion <-> matrix as in diffphys/geom_utils.py:148-203 (quaternions are divided
 * by |q|^2, the best-conditioned of the four matrix->quaternion forms is taken).  a_broadcast != 0: `a` is ONE 7-vector
 * shared by all n elements.  The VJP writes g_a [n][7] (per element also when `a` is broadcast: the caller sums) and
 * g_b [n][6 or 7]; either may be NULL.
 *
 * Pinhole projection of body origins / body-fixed points (the 2D keypoint term; diffphys/dp_utils.py:184-214 parse_rtk,
 * project_bodies), same launch shape, one lane per element:
 *   PD_POSE_PROJECT        a = camera row [16] = the reference's rtk 4x4, row-major: rows 0-2 [R|t] world -> view, row 3
 *                          (fx, fy, cx, cy);  b = pose [n][7], only p is read -> out [n][2] =
 *                          ((fx x + cx z) / z, (fy y + cy z) / z) with (x, y, z) = R p + t.  No clamp: z = 0 gives
 *                          inf / NaN as in the reference.
 *   PD_POSE_PROJECT_POINT  b = [n][10]: a pose followed by a body-frame point c; the projected point is p + R(q) c with
 *                          R(q) as PD_POSE_ROTATE_FRAME forms it (divided by |q|^2).
 * For THESE TWO ops a_broadcast is a group size g, not a flag: g = 0 -- one camera row per element; g >= 1 -- camera row
 * i / g serves element i (g = bodies per (env, frame); g = n: one camera for all).  n % g != 0 (or g < 0) is refused with
 * a pd_last_error text before anything is launched or written.  The VJP writes g_a [n][16] per element, row 3 included
 * (the caller sums over each group), and g_b [n][7] (quaternion entries 0) or [n][10]; either may be NULL.
 *
 * Ground-contact wrench of body states (eval_body_contacts, diffphys/integrator_euler.py:93-179, as a function of ONE state and the
 * materials; the contact materials' gradients and a differentiable grf are built on it -- DESIGN.md section 8):
 *   PD_POSE_GROUND_WRENCH  b = body states [n][13] = (p, q xyzw, w, v): a wp_pos row followed by a wp_vel row, the layout of a resumed
 *                          rollout's state.  a_broadcast = nb (a group size, as above): element i is body i % nb of state set i / nb;
 *                          nb < 1 or n % nb != 0 is refused before anything is launched.  a = ONE contact table for all elements ->
 *                          out [n][6] = the element's contribution to body_f, -sum_c (r_c x f_c, f_c) over the body's touching
 *                          candidates, torque first; zeros for a body without candidates.  Per candidate the arithmetic and the touch
 *                          decision are the rollout kernels' own (csrc/pd_device.h contact_point_fwd / contact_point_adj on a record
 *                          staged like theirs); one wavefront per element sums its candidates in a fixed order (no atomics).
 *                          VJP: g_out [n][6]; g_b [n][13] the raw partials (quaternion entries not projected); g_a [n][nmat][4] the
 *                          gradient of the material rows (ke, kd, kf, mu) PER ELEMENT (the caller sums); either may be NULL, not both.
 * The contact table: a 16-byte-aligned float buffer built on the host (hip_backend.contact_table is the one builder), small integers
 * stored as floats (nc <= 65 535 and nmat <= 255 are exact):
 *   [0..3]                     nb, nc, nmat, 0
 *   [4 .. 4 + 4 nmat)          the material rows (ke, kd, kf, mu)
 *   then 12 floats per body    com.xyz, first candidate, candidate count, bounding sphere of the body's candidates (centre.xyz,
 *                              radius), largest dist, |centre| + radius, the material index that ALL of the body's candidates
 *                              share or -1 (mixed: the material VJP then sweeps once per row)  -- the sphere serves an early-out
 *                              that never drops a touching candidate (bound on the lowest height minus 1 000 roundings of its terms)
 *   then 4 floats per candidate (x, y, z, dist), grouped by body, in template order inside a body
 *   then 1 float per candidate its material index, padded with zeros to a multiple of 4 floats
 * The host cannot validate a device buffer: a table of another model (other nb, nc or nmat than the operands were sized for) is the
 * caller's error, like a numeric-policy mismatch of the rollouts.
 *
 * Joint coordinates of body states -- the inverse of pd_fk_forward (Warp's eval_ik; the numbers the joint pass of a step measures,
 * diffphys/integrator_euler.py:326-445, as outputs -- DESIGN.md section 8):
 *   PD_POSE_JOINT_COORDS   b = body states [n][13] and a_broadcast = nb as for PD_POSE_GROUND_WRENCH (nb < 1 or n % nb != 0 is refused at
 *                          every n; nb <= 256).  a = ONE joint table for all elements -> out [n / nb][nq + nqd], set-major: joint_q [nq]
 *                          then joint_qd [nqd] of each state set, the layouts pd_fk_forward takes.  With the joint frame X_wj = X_parent
 *                          X_p (X_p alone and w_p = v_p = 0 for a body without parent), r_err = conj(q_wj) q_c, w_err = w_c - w_p:
 *                            FREE      q = (R_wj^-1 (p_c - p_wj), r_err),  qd = (R_wj^-1 w_err, R_wj^-1 (v_c - v_p - w_err x com))
 *                            REVOLUTE  q = the twist angle of r_err about the axis (integrator_euler.py:394-400, through atan2: the
 *                                      default numeric policy; the literal-acos policy is not offered for this op),
 *                                      qd = w_err . R_wj axis
 *                            COMPOUND  q = quat_decompose(conj(q_off) r_err q_off) (:411-416); the measured rates m_k = (R_wj R_off a_k)
 *                                      . w_err on the axes a_k of :418-427; rate mode 0 ("measured", what the PD controller sees):
 *                                      qd = m; rate mode 1 ("generalized", the inverse of pd_fk_forward): qd = G^-1 m, G_kj = a_k . a_j
 *                                      (only a_0 . a_2 is off the diagonal; singular at |q_1| = pi / 2)
 *                            FIXED     no coordinates
 *                          One lane per element; every output float is written by exactly one lane (floats of out that belong to no
 *                          joint do not exist: nq and nqd are the sums of the joints' widths).
 *                          VJP: g_out [n / nb][nq + nqd] -> g_b [n][13], the raw partials (quaternion entries not projected).  A body's
 *                          coordinates depend on its own row and on its parent's: whole state sets share a workgroup, every lane leaves
 *                          the parent-side adjoint of its joint in LDS and, after one barrier, adds its children's in the table's child
 *                          order to its own -- no atomics, the same bits on every run.  The table has no gradient: a non-NULL g_a is
 *                          refused.
 * The joint table: a 16-byte-aligned float buffer built on the host (hip_backend.joint_table is the one builder), integers stored as
 * floats:
 *   [0..3]                     nb, nq, nqd, rate mode (0 measured, 1 generalized)
 *   then 24 floats per body    parent (-1: none), joint type, q_start, qd_start, X_p (p.xyz, q.xyzw), axis.xyz, the quaternion of X_c
 *                              (xyzw), com.xyz, number of children, 0, 0
 *   then 8 floats per body     its children in template order, -1 padded (a body with more than 8 children is refused by the builder)
 * As with the contact table, a table of another model is the caller's error.
 *
 * Whole-body (centroidal) quantities of body states -- total mass, centre of mass and its velocity, linear momentum, angular momentum
 * about the centre of mass, kinetic and potential energy, per state set:
 *   PD_POSE_CENTROIDAL     b = rows [n][23] = (p, q xyzw, w, v, m, I row-major 3x3): a state row as for PD_POSE_GROUND_WRENCH (v the
 *                          velocity of the body's centre of mass, w the world angular velocity), the body's mass and its body-frame
 *                          inertia about its centre of mass (the rollouts' body_inertia).  a_broadcast = nb as above (nb < 1 or
 *                          n % nb != 0 is refused at every n; nb <= 256).  a = ONE mass table for all elements -> out [n / nb][16] =
 *                          (M, c.xyz, c_dot.xyz, P.xyz, L.xyz, T, V, 0) of each state set, with x_i = p_i + R(q_i) com_i,
 *                          wb_i = R(q_i)^T w_i (R(q) the map of the quaternion AS IT IS, not normalised, as in the two ops above):
 *                            M = sum m_i     c = sum m_i x_i / M     P = sum m_i v_i     c_dot = P / M
 *                            L = sum [ R(q_i) I_i wb_i + m_i (x_i - c) x (v_i - c_dot) ]       (about the centre of mass)
 *                            T = sum [ m_i |v_i|^2 / 2 + wb_i . I_i wb_i / 2 ]                 V = -sum m_i gravity . x_i
 *                          Whole state sets share a workgroup, a lane per body; two fixed-order tree reductions per set in LDS (first
 *                          M, c, c_dot, P; L is then formed relative to c and c_dot), no atomics: a set's bits depend neither on the
 *                          run nor on n nor on the set's place in the launch.
 *                          VJP: g_out [n / nb][16] (entry 15 is ignored) -> g_b [n][23], the raw partials with respect to the state,
 *                          the mass and the nine inertia entries (no symmetry assumed, quaternion entries not projected).  The table
 *                          has no gradient: a non-NULL g_a is refused, at every n.
 * The mass table: a 16-byte-aligned float buffer built on the host (hip_backend.mass_table is the one builder):
 *   [0..3]                     nb, 0, 0, 0
 *   [4..7]                     gravity.xyz, 0
 *   then 4 floats per body     com.xyz, 0
 * A table whose nb is not the call's a_broadcast is not read beyond its first float: out / g_b are then written as zeros.
 *
 * Ground-contact state of body states -- per body the height of its lowest contact candidate, where that candidate is and how fast
 * it moves, how many candidates touch and how deep:
 *   PD_POSE_CONTACT_STATE  b = body states [n][13] and a_broadcast = nb as for PD_POSE_GROUND_WRENCH (nb < 1 or n % nb != 0 is refused at
 *                          every n; any nb).  a = the contact table of PD_POSE_GROUND_WRENCH, unchanged (its material rows and
 *                          bounding spheres are not read) -> out [n][8] = (h, x, z, u.x, u.y, u.z, s, k).  Per candidate c of the
 *                          body, P_c = (x, y, z, dist), with the quaternion AS IT IS (not normalised) and R = its linear map:
 *                            h_c = p.y + (row 1 of R) . P_c.xyz - dist_c     the rollouts' height and touch decision !(h_c > 0),
 *                                                                             bit for bit (csrc/pd_math.h contact_height)
 *                            rp = R P_c.xyz      rc = R com      rr_c = (rp.x - rc.x, h_c - p.y - rc.y, rp.z - rc.z)
 *                            u_c = v + w x rr_c                                           (cp, rr, dpdt of contact_point_fwd)
 *                          c* = the candidate of lowest h_c, lowest table index on ties: h = h_c*, (x, z) = (p.x + rp*.x,
 *                          p.z + rp*.z), u = u_c*;
 *                          k = the number of touching candidates, stored as a float; s = the sum of -h_c over them.  A body
 *                          without candidates gives (+inf, 0, 0, 0, 0, 0, 0, 0).  A row with a non-finite entry may give anything
 *                          in its own element; it reads nothing out of range and disturbs no other element.  One wavefront per
 *                          element sweeps ALL the body's candidates (no early-out: the height is wanted for bodies in the air),
 *                          then a fixed-order butterfly: no atomics, the same bits on every run, at every n and place in the launch.
 *                          VJP: g_out [n][8] (entry 7, the count's, is ignored) -> g_b [n][13], the raw partials (quaternion
 *                          entries not projected): through c*, found again with the same bits, and through s.  Zeros for a body
 *                          without candidates.  The table has no gradient: a non-NULL g_a is refused, at every n.
 * A table whose nb is not the call's a_broadcast, or a candidate range that leaves the table's nc, reads no candidate: the element is
 * then a body without candidates.
 *
 * Joint wrench of body states -- per body what the joint pass of a step adds to body_f: the PD force, the limit force and the attachment
 * springs of its own joint and of its children's (eval_body_joints, diffphys/integrator_euler.py:289-451, as a function of ONE state and
 * the joints' controls; a differentiable jaf is built on it -- DESIGN.md section 8):
 *   PD_POSE_JOINT_WRENCH   b = rows [n][25]: a state row as for PD_POSE_GROUND_WRENCH, then the controls of this body's joint in dof
 *                          slots k = 0..2: act[k] at 13 + k, target[k] at 16 + k, ke[k] at 19 + k, kd[k] at 22 + k.  A REVOLUTE joint
 *                          uses slot 0, a COMPOUND joint slots 0..2, FREE and FIXED joints none; an unused slot never enters
 *                          arithmetic (it may hold anything) and its gradient is written as 0.  a_broadcast = nb as above (nb < 1 or
 *                          n % nb != 0 is refused at every n; nb <= 256).  a = ONE joint-force table for all elements -> out [n][6] =
 *                          (torque, force) per body.  Joint i (= child body i, frames and errors as for PD_POSE_JOINT_COORDS) makes
 *                          the pair (t_i, f_i), with ake / akd the attachment gains, ads = 0.01, x_err = (p_c - p_p) - R(q_p) p_pj
 *                          (p_c - p_pj without parent), v_err = v_c - v_p, r_c = -R(q_c) com_c, r_p = R(q_p) (p_pj - com_p):
 *                            FIXED     t = R(q_wj) ang_err ake + w_err akd ads, ang_err = normalize(r_err.xyz) 2 acos(r_err.w) in its
 *                                      scale-invariant form (2 atan2(|v|, w) / |v|, series near 0: finite at the identity)
 *                            REVOLUTE  t = axis_p jf + (axis_p x axis_c) ake + (w_err - axis_p qd) akd ads, with axis_p = R(q_wj) axis,
 *                                      axis_c = R(q_c) axis, q the twist angle (through atan2), qd = w_err . axis_p and
 *                                      jf = ke (q - target) + kd qd + act - limit force(q, qd) (integrator_euler.py:261-286)
 *                            COMPOUND  t = clamp(sum_k axw_k jf_k, +-1e4) per component on the angles, world axes axw_k = R_wj R_off a_k
 *                                      and measured rates of PD_POSE_JOINT_COORDS (rate mode 0), jf_k as above for slot k
 *                            f = x_err ake + v_err akd   (COMPOUND: clamped to +-1e4 per component);   FREE: no pair
 *                          out_i = -(t_i + r_c,i x f_i, f_i) + sum over the children c of i, in the table's child order, of
 *                          (t_c + r_p,c x f_c, f_c): what a rollout step adds to body_f for that state and those controls (its jaf;
 *                          the same function in fp32, not the same bits -- the lever arms and x_err are formed here without the
 *                          cancellation of two numbers of the size of the body's distance from the origin).  The default numeric
 *                          policy only.  Whole state sets share a workgroup, a lane per body; a lane leaves the parent-side wrench of
 *                          its joint in LDS and, after one barrier, adds its children's to its own side: no atomics, a set's bits
 *                          depend neither on the run nor on n nor on the set's place in the launch.
 *                          VJP: g_out [n][6] -> g_b [n][25], the raw partials with respect to the state (quaternion entries not
 *                          projected) and the twelve control slots; a clamped component passes no gradient.  Limits, attachment
 *                          gains and the table have no gradient: a non-NULL g_a is refused, at every n.
 * The joint-force table: a 16-byte-aligned float buffer built on the host (hip_backend.joint_force_table is the one builder): the joint
 * table above with rate mode 0, float for float (4 + 32 nb floats), followed by
 *   4 floats                   attach_ke, attach_kd, 0, 0
 *   then 12 floats per body    (lower, upper, limit_ke, limit_kd) of dof slots 0..2 = the template's joint_limit_*[qd_start + k];
 *                              (-FLT_MAX, FLT_MAX, 0, 0) in a slot no dof uses
 * A table whose nb is not the call's a_broadcast is not read beyond its first float: out / g_b are then written as zeros.  A parent
 * index or a coordinate range outside the set is handled as for PD_POSE_JOINT_COORDS.
 *
 * Generalised joint forces of body wrenches -- the transpose of the articulation's Jacobian: the torque about every hinge axis and the
 * net wrench on a floating root that a set of per-body wrenches (a grf, jaf or body_f row per body) amounts to:
 *   PD_POSE_GENERALIZED_FORCE  b = rows [n][13] = (p, q xyzw, t, f): the pose of a state row followed by the body's wrench, torque
 *                          first, world axes, the force acting at the body's centre of mass.  Velocities are not an input.
 *                          a_broadcast = nb as above (nb < 1 or n % nb != 0 is refused at every n; nb <= 256).  a = ONE joint table of
 *                          PD_POSE_JOINT_COORDS, unchanged, for all elements; its mode float [3] selects the effort convention of
 *                          COMPOUND joints -> out [n / nb][nqd], set-major, in the joint_qd layout.  With x_b = p_b + R(q_b) com_b
 *                          (R(q) the map of the quaternion AS IT IS), the subtree sums F_i = sum f_b and N_i(o) = sum (t_b +
 *                          (x_b - o) x f_b) over the bodies b of the subtree of body i, and the joint frame (p_wj, q_wj) and world
 *                          axes axw_k = R_wj R_off a_k (angles from the poses) of PD_POSE_JOINT_COORDS:
 *                            REVOLUTE  tau = (R_wj axis) . N_i(p_wj)
 *                            COMPOUND  g_k = axw_k . N_i(p_wj); mode 1 ("generalized"): tau_k = g_k, conjugate to the generalised
 *                                      rates (sum tau_k qd_k = N . w_err); mode 0 ("actuator"): tau = G^-1 g, G_kj = a_k . a_j -- the
 *                                      Gram solve of the rates, singular at |q_1| = pi / 2 --, conjugate to the measured rates: the
 *                                      efforts jf_k for which sum axw_k jf_k has these projections, the units of torques and of
 *                                      the PD force
 *                            FREE      (R_wj^-1 N_i(x_i), R_wj^-1 F_i): the net wrench on the subtree, the moment about the child
 *                                      body's centre of mass -- conjugate to that body's twist (w, v) under rigid motion of the
 *                                      subtree.  It is NOT conjugate to PD_POSE_JOINT_COORDS' FREE linear rate, which carries Warp's
 *                                      unrotated-com lever (v_c - v_p - w_err x com).
 *                            FIXED     no output
 *                          Every float of out is written by exactly one lane.  Whole state sets share a workgroup, a lane per body.
 *                          The bodies' depths come from the table's parent indices (pointer jumping in LDS); the subtree sums go
 *                          through LDS level by level, deepest first, every body adding its children in the table's child order; the
 *                          moments are accumulated about the origin of the set's body 0 and moved to each anchor afterwards, so the
 *                          set's distance from the world origin does not enter.  No atomics: a set's bits depend neither on the run
 *                          nor on n nor on the set's place in the launch.
 *                          VJP: g_out [n / nb][nqd] -> g_b [n][13], the raw partials with respect to pose and wrench (quaternion
 *                          entries not projected): the mirror image, an ancestor sum from the roots down, then the parent-side pose
 *                          adjoints gathered as for PD_POSE_JOINT_COORDS.  The table has no gradient: a non-NULL g_a is refused, at
 *                          every n.
 * A table whose nb is not the call's a_broadcast is not read beyond its header: out [n / nb][nqd of THAT header] / g_b are then
 * written as zeros.  A parent index or a coordinate range outside the set is handled as for PD_POSE_JOINT_COORDS.
 *
 * Rigid-body twists of joint rates -- the articulation's Jacobian applied to joint rates, the conjugate of PD_POSE_GENERALIZED_FORCE:
 * the twist (w, v) every body has when the joints move at those rates and the links are rigid:
 *   PD_POSE_BODY_TWIST     b = rows [n][13] = (p, q xyzw, r_0..r_5): the pose of a state row followed by the rates of THIS body's joint
 *                          in six slots, slot k = joint_qd[qd_start + k] for k below the joint's dof count (6 FREE, 3 COMPOUND,
 *                          1 REVOLUTE, 0 FIXED); a further slot never enters arithmetic and its gradient is written as 0.
 *                          a_broadcast = nb as above (nb < 1 or n % nb != 0 is refused at every n; nb <= 256).  a = ONE joint table of
 *                          PD_POSE_JOINT_COORDS, unchanged, for all elements; its mode float [3] selects the rate convention of
 *                          COMPOUND joints (0 measured, 1 generalized) -> out [n][6] = (w, v) per body, world axes, v the velocity of
 *                          the body's centre of mass x_b = p_b + R(q_b) com_b.  On the frames, axes and anchors of
 *                          PD_POSE_GENERALIZED_FORCE, per joint i:
 *                            REVOLUTE  w_i = (R_wj axis) r_0                 u_i = 0              o_i = p_wj
 *                            COMPOUND  w_i = sum_k axw_k rho_k               u_i = 0              o_i = p_wj;  mode 1: rho = r; mode 0:
 *                                      rho = G^-1 r, the Gram solve of the rates (singular at |q_1| = pi / 2)
 *                            FREE      w_i = R_wj r_0..2                     u_i = R_wj r_3..5    o_i = x_i, the child's centre of mass
 *                            FIXED     nothing
 *                          w_b = sum w_i and v_b = sum (u_i + w_i x (x_b - o_i)) over the joints of b and of its ancestors: the exact
 *                          transpose of PD_POSE_GENERALIZED_FORCE in each mode (sum tau . r = sum wrench . twist).  The FREE linear
 *                          slots are R_wj^-1 of the centre-of-mass velocity the joint contributes, NOT PD_POSE_JOINT_COORDS' FREE
 *                          linear rate.  A lane per body, whole state sets per workgroup; the ancestor sums go through LDS level by
 *                          level from the roots down, every lever formed from differences about the origin of the set's body 0.  No
 *                          atomics: a set's bits depend neither on the run nor on n nor on the set's place in the launch.
 *                          VJP: g_out [n][6] -> g_b [n][13], the raw partials with respect to pose and rate slots (quaternion entries
 *                          not projected): the ancestor sum of w again, subtree sums of the twists' adjoints, the joint's adjoint and
 *                          the parent-side pose adjoints gathered as for PD_POSE_JOINT_COORDS.  The table has no gradient: a
 *                          non-NULL g_a is refused, at every n.
 * A table whose nb is not the call's a_broadcast is not read beyond its first float: out / g_b are then written as zeros.  A parent
 * index or a coordinate range outside the set is handled as for PD_POSE_JOINT_COORDS.
 *
 * Body accelerations of a state -- J qdd + Jdot qd of the articulation, the second-order term next to PD_POSE_BODY_TWIST (DESIGN.md
 * section 8):
 *   PD_POSE_BODY_ACCEL     b = rows [n][19] = (p, q xyzw, w, v, s_0..s_5): a state row as for PD_POSE_JOINT_COORDS (w the world angular
 *                          velocity, v the velocity of the body's centre of mass) followed by the TIME DERIVATIVES of the rate slots of
 *                          THIS body's joint, in PD_POSE_BODY_TWIST's slot layout (slot k = dof qd_start + k below the joint's dof
 *                          count; a further slot never enters arithmetic and its gradient is written as 0).  a_broadcast = nb and
 *                          a = ONE joint table of PD_POSE_JOINT_COORDS as above; its mode float [3] says in which convention the
 *                          COMPOUND slots are read (1 generalized, 0 measured) -> out [n][6] = (alpha, a) per body, world axes, a the
 *                          acceleration of the body's centre of mass x_b = p_b + R(q_b) com_b.  State-based: every velocity-dependent
 *                          term comes from the row's own twist and its parent's; no joint rates are passed.  With pi the parent of
 *                          joint i (w_pi = v_pi = 0 and a constant frame without one), o0 the origin of the set's body 0, d_b = x_b - o0:
 *                            every joint  om_i = w_i - w_pi
 *                            REVOLUTE  omd_i = (R_wj axis) s_0 + w_pi x om_i      ud_i = 0     o_i = p_wj,
 *                                      od_i = v_pi + w_pi x (p_wj - x_pi)  (0 without a parent)
 *                            COMPOUND  ah_k = R_wj R_off a_k, m_k = ah_k . om_i, rho = G^-1 m (the Gram solve of PD_POSE_JOINT_COORDS'
 *                                      generalized rates, s = a_0 . a_2, in EITHER mode);  mode 1: rhod = s_0..2;  mode 0:
 *                                      rhod = G^-1 (s_0 - sd rho_2, s_1, s_2 - sd rho_0), sd = rho_1 a_0 . (a_1 x a_2)
 *                                      omd_i = sum_k ah_k rhod_k + w_pi x om_i + rho_0 rho_1 ah_0 x ah_1 + rho_0 rho_2 ah_0 x ah_2
 *                                              + rho_1 rho_2 ah_1 x ah_2;   ud_i = 0, o_i and od_i as REVOLUTE
 *                            FREE      u_i = v_i - v_pi - w_pi x (x_i - x_pi)
 *                                      omd_i = R_wj s_0..2 + w_pi x om_i    ud_i = R_wj s_3..5 + w_pi x u_i    o_i = x_i, od_i = v_i
 *                            FIXED     omd_i = w_pi x om_i, ud_i = 0, anchor as REVOLUTE  (om_i is 0 on a rigid state)
 *                            e_i = ud_i - omd_i x (o_i - o0) - om_i x od_i
 *                          alpha_b = sum omd_i and a_b = sum e_i + alpha_b x d_b + w_b x v_b, the sums over the joints of b and of
 *                          its ancestors.  On a rigid state (twists = PD_POSE_BODY_TWIST of its joint rates) this is the exact time
 *                          derivative of PD_POSE_BODY_TWIST's output along the motion whose slot rates change at s; on any other
 *                          state it is this formula.  Every lever is a difference about o0.  Mapping, sweeps and the bit guarantees
 *                          are PD_POSE_BODY_TWIST's.
 *                          VJP: g_out [n][6] -> g_b [n][19], the raw partials with respect to the whole row (quaternion entries not
 *                          projected): the ancestor sum again, subtree sums of the accelerations' adjoints, the joint's adjoint, and
 *                          the parent-side adjoint -- a whole state row, 13 floats: the parent's pose and twist both enter -- gathered
 *                          in the table's child order.  The table has no gradient: a non-NULL g_a is refused, at every n.
 * A table of another nb, a parent index or a coordinate range outside the set: as for PD_POSE_BODY_TWIST.
 *
 * The inverse of the mass matrix of a state, applied to a joint-space vector -- the articulated-body recursion:
 *   PD_POSE_MASS_INVERSE   b = rows [n][23] = (p, q xyzw, m, I row-major 3x3, r_0..r_5): the body's pose, its mass, its body-frame
 *                          inertia about the centre of mass (as in PD_POSE_CENTROIDAL's rows; its symmetric part enters) and the
 *                          joint-space force entries of THIS body's joint in PD_POSE_BODY_TWIST's slot layout -- the efforts
 *                          conjugate to the table's rate mode; a further slot never enters arithmetic.  a_broadcast = nb (at most 256)
 *                          and a = ONE joint table of PD_POSE_JOINT_COORDS as above, its mode float [3] included -> out [n][6] =
 *                          the solution x in the same slots, 0 in a slot no dof uses:
 *                            J = PD_POSE_BODY_TWIST's Jacobian in the table's mode,  M_b = diag(R_b I_b R_b^T, m_b 1),
 *                            H = sum_b J_b^T M_b J_b,   out = H^-1 r   per state set.
 *                          In mode 1 (generalized) H is the mass matrix of the generalised rates; in mode 0 (measured) the COMPOUND
 *                          columns are Ah G^-1, exactly as PD_POSE_BODY_TWIST reads its rates.  Recursion, in world axes about o0 = the
 *                          origin of the set's body 0, spatial vectors (angular, linear at o0), d_b = x_b - o0, r_i = the joint's
 *                          anchor - o0:  spatial inertia [[Ibar - m [d]x[d]x, m [d]x], [-m [d]x, m 1]], Ibar = R sym(I) R^T;  motion
 *                          subspace S_i = REVOLUTE (ah, -ah x r_i), COMPOUND three such columns, FREE (R_wj e_k, -R_wj e_k x d_b) and
 *                          (0, R_wj e_k), FIXED none.  Up, deepest level first: IA = I_b + sum Ia_c, pA = sum pa_c, U = IA S,
 *                          D = S^T U = L diag(dd) L^T, W = L^-1 U^T, z = L^-1 (r_b - S^T pA); the body hands up
 *                          Ia = IA - W^T dd^-1 W (exactly 0 behind a 6-dof joint) and pa = pA + W^T dd^-1 z; a body without a dof
 *                          hands IA, pA up unchanged.  Down, from the roots: x_b = L^-T dd^-1 (z - W a_pi), a_b = a_pi + S x_b.
 *                          D is factored, never inverted.  A pivot that is not positive (a massless body on a joint with dofs: a
 *                          singular H) gives inf / NaN; a massless body on a FIXED joint is fine.  O(nb) per set, one launch, no
 *                          atomics: a set's bits depend neither on the run nor on n nor on its place in the launch.
 *                          GRADIENT: there is no VJP kernel.  pd_pose_op_vjp refuses this code at every n, after the shared checks
 *                          (n % g, the cap, g_a), and says so in pd_last_error; nothing is launched or written.  H is symmetric, so the
 *                          op is self-adjoint in its slots and the caller composes the gradient: with lam = pd_pose_op(21) of
 *                          g_out in place of r, the gradient in r is lam, and the gradient in poses, masses and inertias is that of
 *                            - sum_b tlam_b . M_b(q_b, m_b, I_b) . tx_b,   tx = PD_POSE_BODY_TWIST(pose, x),  tlam = PD_POSE_BODY_TWIST(pose, lam)
 *                          in the table's mode with x and lam held constant: one more launch of this op, one PD_POSE_BODY_TWIST on
 *                          the 2 S stacked sets, its VJP, and M_b's own partials (dp_model.MassInverse does exactly that).
 * A table of another nb: out is written as zeros, no row of the table is read.  A parent index or a coordinate range outside the set:
 * as for PD_POSE_BODY_TWIST -- a malformed table never indexes outside the set.
 *
 * The joint-space mass matrix of a state -- the composite-rigid-body recursion:
 *   PD_POSE_MASS_MATRIX    b = rows [n][17] = (p, q xyzw, m, I row-major 3x3): pose, mass and body-frame inertia about the centre of
 *                          mass as in PD_POSE_MASS_INVERSE's rows (the symmetric part of I enters).  a_broadcast = nb (at most 256)
 *                          and a = ONE joint table of PD_POSE_JOINT_COORDS, byte for byte, its mode float [3] included ->
 *                          out [n / nb][nqd * nqd], row-major, in the joint_qd layout (the table's dof starts):
 *                            H = sum_b J_b^T diag(R_b sym(I_b) R_b^T, m_b 1) J_b,   J = PD_POSE_BODY_TWIST's Jacobian in the table's mode
 *                          -- in mode 1 (generalized) the mass matrix of the generalised rates, in mode 0 (measured) the matrix whose
 *                          inverse PD_POSE_MASS_INVERSE applies in that mode.  In PD_POSE_MASS_INVERSE's frame, spatial inertias I_b
 *                          and motion subspaces S_i:  up, deepest level first, Ic_i = I_i + sum_children Ic_c (the table's child
 *                          order);  F_i = Ic_i S_i;  walking j = i, parent(i), ...: H[dofs_j, dofs_i] = S_j^T F_i and its transpose.
 *                          An entry between dofs of two bodies neither of which is the other's ancestor is exactly 0.0f; out[a][b]
 *                          and out[b][a] are the same bits.  One launch, no atomics: a set's bits depend neither on the run nor on
 *                          n nor on its place in the launch.  fp32 rows, frames and S; inertias, sums and products in double.
 *                          VJP: g_out [n / nb][nqd * nqd], arbitrary (not assumed symmetric) -> g_b [n][17], the raw partials in
 *                          pose, mass and inertia (quaternions as they are; the inertia's are those of sym(I)), by a kernel of its
 *                          own: with Gs = (g_out + g_out^T) / 2, A_i = sum_{j in anc*(i)} S_j Gs_ji,
 *                          dL/dI_b = sum_{i in anc*(b)} (A_i S_i^T + S_i A_i^T - S_i Gs_ii S_i^T),
 *                          dL/dS_i = 2 (Ic_i A_i + sum_{k in desc(i)} F_k Gs_ki), chained into the rows; contributions to a parent's
 *                          row are gathered in the table's child order.  The table has no gradient: a non-NULL g_a is refused, at
 *                          every n.
 * A table of another nb: zeros, no row of the table is read; a malformed table never indexes outside the set (a walk over parents is
 * bounded by nb steps).
 *
 * No allocation, no synchronisation: capturable in a HIP graph.  n = 0 is legal.  A refused call returns non-zero and
 * leaves its reason in pd_last_error.  PD_POSE_GROUND_WRENCH, PD_POSE_JOINT_COORDS, PD_POSE_CENTROIDAL, PD_POSE_CONTACT_STATE,
 * PD_POSE_JOINT_WRENCH, PD_POSE_GENERALIZED_FORCE, PD_POSE_BODY_TWIST, PD_POSE_BODY_ACCEL, PD_POSE_MASS_INVERSE and PD_POSE_MASS_MATRIX are new op
 * codes of the two entries: no symbol or signature changed, the version stays 9.  The enum has gaps: codes 7, 8, 10, 12, 14, 16, 18, 20
 * and 22 are not assigned and are refused as "unknown op", and so is 24, the code after the last -- callers and tests of version 9 rely
 * on that refusal (of 7 and 8 since the centroidal op took 9, of 10 since the contact state took 11, of 12 since the joint wrench took
 * 13, of 14 since the generalised force took 15, of 16 since the body twist took 17, of 18 since the body acceleration took 19, of 20
 * since the mass inverse took 21, of 22 since the mass matrix took 23), so the nine stay free for as long as the version is 9. */
enum { PD_POSE_COMPOSE_DELTA = 0, PD_POSE_ROTATE_FRAME = 1, PD_POSE_ROTATE_VEL = 2, PD_POSE_PROJECT = 3, PD_POSE_PROJECT_POINT = 4,
       PD_POSE_GROUND_WRENCH = 5, PD_POSE_JOINT_COORDS = 6, PD_POSE_CENTROIDAL = 9, PD_POSE_CONTACT_STATE = 11,
       PD_POSE_JOINT_WRENCH = 13, PD_POSE_GENERALIZED_FORCE = 15, PD_POSE_BODY_TWIST = 17,
       PD_POSE_BODY_ACCEL = 19, PD_POSE_MASS_INVERSE = 21, PD_POSE_MASS_MATRIX = 23 };
int pd_pose_op(int op, int n, const float *a_dev, int a_broadcast, const float *b_dev, float *out_dev, void *stream);
int pd_pose_op_vjp(int op, int n, const float *a_dev, int a_broadcast, const float *b_dev, const float *g_out_dev,
                   float *g_a_dev, float *g_b_dev, void *stream);

/* Lowest ground-contact candidate of each of n pose sets (get_foot_height / the reg_foot term, diffphys/dp_model.py:
 * 574-579,762,814, evaluated on the contact candidates instead of posed visual meshes):  height[i] = min over candidates c of
 * body_q[i][c_body[c]].p.y + (R(body_q[i][c_body[c]].q) c_point[c]).y - c_dist[c];  arg[i] = the minimising candidate
 * (lowest index on ties).  body_q [n][nb][7].  The VJP writes g_body_q [n][nb][7] (zero except the arg-min body). */
int pd_foot_height(int n, int nb, int nc, const float *body_q_dev, const int *c_body_dev, const float *c_point_dev,
                   const float *c_dist_dev, float *height_dev, int *arg_dev, void *stream);
int pd_foot_height_vjp(int n, int nb, const float *body_q_dev, const int *c_body_dev, const float *c_point_dev,
                       const int *arg_dev, const float *g_height_dev, float *g_body_q_dev, void *stream);

/* out[c] = sum over the n rows of x[n][k] (row-major), rows added in a fixed order: the bias gradient of the time-MLPs' linear layers
 * (reference: torch's autograd of nn.Linear in diffphys/lab4d_utils.py BaseMLP) and the gradient of an operand that was broadcast over
 * n poses (global_q in rotate_frame, diffphys/dp_utils.py:113-138) -- as one launch that gives the same bits eagerly and in a replayed
 * HIP graph.  n = 0 writes zeros.  ws_dev: PD_COLSUM_SLICES * k floats of caller-owned scratch (row slices are summed there first, then the
 * slices in order); NULL, or n <= 1024: one slice, one launch -- the result of a given (n, k, ws given or not) never depends on anything else. */
#define PD_COLSUM_SLICES 32
int pd_colsum(int n, int k, const float *x_dev, float *out_dev, float *ws_dev, void *stream);

/* Weight and bias gradient of a linear layer y = x W^T + b over n samples, on the fp32 matrix cores (csrc/pd_mlp.hip):
 *   gw[m][kin] = sum_s g[s][m] x[s][kin],   gb[m] = sum_s g[s][m]   (gb_dev may be NULL)
 * g_dev [n][m] = dL/dy, x_dev [n][kin], row-major, contiguous.  Fixed summation order: the same bits on every call, eagerly and in a replayed
 * HIP graph.  Reference: torch autograd of nn.Linear in the time-MLPs (diffphys/lab4d_utils.py BaseMLP / TimeMLP; torch_utils.py:116-180) at
 * the training window of main.py:86 (n = 7 600).  Shapes: m and kin multiples of 128; pd_linear_wgrad_workspace_floats returns 0 for any other
 * shape (the caller keeps its BLAS path) and otherwise the floats of caller-owned scratch ws_dev needs. */
size_t pd_linear_wgrad_workspace_floats(int n, int m, int kin);
int pd_linear_wgrad(int n, int m, int kin, const float *g_dev, const float *x_dev, float *gw_dev, float *gb_dev, float *ws_dev, void *stream);

/* Device time (ms) of this model's last `kind` launch, measured with hipEvents recorded on the launch stream around
 * the kernel: kind 0 = rollout forward, 1 = rollout backward.  Enabled per model by pd_model_set_timing(m, 1); used by
 * bench.py.  Returns a negative value when nothing was timed.  (Synchronises on the end event.) */
int pd_model_set_timing(pd_model *m, int on);
float pd_last_kernel_ms(const pd_model *m, int kind);

/* Launch geometry of the last rollout launch of `kind` on this model (bench.py reports it beside the roofline):
 * out[0] workgroups, out[1] threads per workgroup, out[2] dynamic LDS bytes per workgroup, out[3] envs per workgroup.
 * kind PD_LAUNCH_INFO_PARENT_FRAMES (see pd_model_set_kernel_family): out[0] 1 when the robot qualifies for the adjoint kernels of unrotated
 * parent-side joint frames, out[1] the setting (0 automatic, 1 general, 2 specialised), out[2] 1 when the last adjoint launch ran them,
 * out[3] the model facts: 1 when the robot qualifies for having them compiled in + 2 when PD_PFI_NO_FACTS is set + 4 when the last adjoint
 * launch ran the kernels with the facts compiled in; the com facts in the same way: + 8 when the robot qualifies, + 16 when
 * PD_PFI_NO_COM_FACTS is set, + 32 when the last adjoint launch ran the kernels with them compiled in. */
#define PD_LAUNCH_INFO_PARENT_FRAMES 2
int pd_last_launch_info(const pd_model *m, int kind, int out[4]);

#ifdef __cplusplus
}
#endif
#endif
