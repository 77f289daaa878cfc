/*
 * pianosim.h - C-ABI of the MI355X batched PianoWithShadowHands environment.
 *
 * The reference has no FFI for this path: its boundary is the Python VecEnv
 * `parallelized_base_v2.VectorizedPianoEnv` (parallelized_base_v2.py:21-67), whose
 * per-env work is dm_control `composer.Environment.step/reset` driving MuJoCo
 * `mj_step` on a `PianoWithShadowHands` task (robopianist/suite/tasks/
 * piano_with_shadow_hands.py:49-449). These entry points are what that VecEnv binds
 * (see INTEGRATION.md for the ctypes stub):
 *
 *   ps_create        <- VectorizedPianoEnv.__init__ (parallelized_base_v2.py:22-46):
 *                       builds N tasks + physics (tasks/base.py:45-197,
 *                       piano_with_shadow_hands.py:98-128).
 *   ps_reset         <- VectorizedPianoEnv.reset (parallelized_base_v2.py:48-51) ->
 *                       composer reset: mj_resetData + initialize_episode
 *                       (piano_with_shadow_hands.py:169-174, piano.py:145-152).
 *   ps_step          <- VectorizedPianoEnv.step (parallelized_base_v2.py:53-60) ->
 *                       before_step (:176-186), 10 x mj_step + Piano.after_substep
 *                       (piano.py:154-192), after_step (:188-204), observables
 *                       (:371-449), CompositeReward.compute (composite_reward.py:46-56),
 *                       termination (:213-220), auto-reset after LAST.
 *   ps_get_state /   <- physics.data.qpos/qvel/qacc_warmstart/ctrl + task._t_idx
 *   ps_set_state        (teacher-forced parity; no reference equivalent beyond
 *                       physics.set_state).
 *   ps_set_applied   <- physics.bind(joints).qfrc_applied (piano_with_shadow_hands_test.py:239).
 *   ps_reward_terms  <- CompositeReward.reward_terms (composite_reward.py:62-64).
 *   ps_musical_metrics <- MidiEvaluationWrapper (wrappers/evaluation.py:37-177): per-step
 *                       precision / recall / F1 of the key and sustain activations against
 *                       the notes of the step, averaged over each finished episode.
 *
 * Conventions: all array arguments of ps_reset/ps_step/ps_get_state/ps_set_state are
 * DEVICE pointers (e.g. torch-ROCm tensors' data_ptr()) and the calls are asynchronous
 * on the caller's HIP stream (`stream` = hipStream_t, NULL = default stream). Return
 * value 0 = OK, < 0 = error; ps_last_error() gives a thread-local message. No C++
 * exception crosses the ABI. One handle per device; handles are independent.
 */
#ifndef PIANOSIM_H
#define PIANOSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- fixed topology (robopianist: 88-key piano + 2 Shadow Hand E3M5 + 2 forearm DOFs) */
#define PS_NKEY 88          /* piano_constants.py:22 */
#define PS_NHAND 2          /* right, left (tasks/base.py:116-135) */
#define PS_HAND_NBODY 25    /* forearm + wrist + palm + 4x4 fingers(+lf metacarpal) + 5 thumb */
#define PS_HAND_NDOF 26     /* shadow_hand_constants.py:21 NQ=24, + forearm_tx/ty */
#define PS_HAND_NGEOM 20    /* authored capsule colliders per hand */
#define PS_HAND_NACT 22     /* shadow_hand_constants.py:22 NU=20, + 2 forearm position actuators */
#define PS_HAND_NTENDON 4   /* FFJ0, MFJ0, RFJ0, LFJ0 fixed tendons */
#define PS_NFINGER 5        /* fingertip sites th, ff, mf, rf, lf (shadow_hand_constants.py:33-40) */
#define PS_NV (PS_NKEY + PS_NHAND * PS_HAND_NDOF)     /* 140 */
#define PS_NU (PS_NHAND * PS_HAND_NACT)               /* 44 */
#define PS_NACTION (PS_NU + 1)                        /* 45: hands + sustain */
#define PS_MAX_CAPPAIRS 768 /* capsule-capsule candidate pairs after filtering */
/* Box and convex-hull hand colliders ("extra" geoms, beside the capsule slots): MuJoCo geom
 * types box and mesh (the Menagerie hand's palm boxes and distal meshes, shadow_hand.py:95,
 * 144-152). A mesh collides as the convex hull of its vertices, as in MuJoCo. */
#define PS_HAND_NXGEOM 12      /* extra colliders per hand */
#define PS_HULL_MAXVERT 64     /* vertices of one hull */
#define PS_HAND_HULLVERT 384   /* hull vertices per hand, all hulls */
#define PS_MAX_XPAIRS 1024     /* hand-hand candidate pairs that involve an extra collider */
#define PS_GEOM_NONE 0
#define PS_GEOM_BOX 1
#define PS_GEOM_HULL 2
#define PS_MAX_NOTES 16     /* notes per control step in the song tables */

/* Per-geom contact parameters (MuJoCo geom attributes). */
typedef struct {
  double solref[2];   /* timeconst, dampratio */
  double solimp[5];   /* d0, dwidth, width, midpoint, power */
  double friction;    /* sliding friction (condim 3, pyramidal) */
} ps_contact_param;

/* Compiled model ("mjModel" for this task), produced by the host model compiler
 * (diffusion-piano_amd/model.py). Lengths in metres, angles in radians. */
typedef struct {
  double timestep;          /* tasks/base.py:28 */
  int32_t n_substeps;       /* control 0.05 / physics 0.005 (tasks/base.py:28-31) */
  double gravity[3];
  /* piano keys (piano_mjcf.py:64-400), sorted by key number */
  double key_pos[PS_NKEY][3];      /* body position (world) */
  double key_half[PS_NKEY][3];     /* box half sizes */
  double key_anchor[PS_NKEY][3];   /* hinge position in the key body frame */
  double key_mass[PS_NKEY];
  double key_inertia[PS_NKEY];     /* moment of inertia about the hinge axis (no armature) */
  double key_armature[PS_NKEY];
  double key_damping[PS_NKEY];
  double key_stiffness[PS_NKEY];
  double key_springref[PS_NKEY];
  double key_range[PS_NKEY][2];
  double base_pos[3], base_half[3];  /* static piano base box */
  ps_contact_param piano_contact;
  double limit_solref[2], limit_solimp[5];
  /* hands: [0]=right, [1]=left. Bodies in MuJoCo tree order; parent -1 = world. */
  int32_t body_parent[PS_NHAND][PS_HAND_NBODY];
  double body_pos[PS_NHAND][PS_HAND_NBODY][3];   /* in parent frame */
  double body_quat[PS_NHAND][PS_HAND_NBODY][4];  /* w x y z, in parent frame */
  double body_mass[PS_NHAND][PS_HAND_NBODY];
  double body_ipos[PS_NHAND][PS_HAND_NBODY][3];  /* COM in body frame */
  double body_inertia[PS_NHAND][PS_HAND_NBODY][6]; /* about COM, body frame: xx yy zz xy xz yz */
  /* DOFs in MuJoCo qpos order (each hinge/slide at its body origin). */
  int32_t dof_body[PS_NHAND][PS_HAND_NDOF];
  int32_t dof_type[PS_NHAND][PS_HAND_NDOF];     /* 0 = hinge, 1 = slide */
  double dof_axis[PS_NHAND][PS_HAND_NDOF][3];   /* body frame */
  double dof_range[PS_NHAND][PS_HAND_NDOF][2];
  int32_t dof_limited[PS_NHAND][PS_HAND_NDOF];
  double dof_damping[PS_NHAND][PS_HAND_NDOF];
  double dof_armature[PS_NHAND][PS_HAND_NDOF];
  int32_t dof_obs_order[PS_NHAND][PS_HAND_NDOF]; /* joints_pos[i] = qpos[dof_obs_order[i]] */
  /* capsule colliders (body frame segment centre/axis); geom_body < 0: unused slot */
  int32_t geom_body[PS_NHAND][PS_HAND_NGEOM];
  double geom_pos[PS_NHAND][PS_HAND_NGEOM][3];
  double geom_axis[PS_NHAND][PS_HAND_NGEOM][3];
  double geom_halflen[PS_NHAND][PS_HAND_NGEOM];
  double geom_radius[PS_NHAND][PS_HAND_NGEOM];
  int32_t root_geom_count;   /* capsules [0, root_geom_count) belong to the root (forearm) body
                                (informational: the forearm reward tests the bodies) */
  ps_contact_param hand_contact;
  /* fingertip sites (shadow_hand.py:190-207) */
  int32_t site_body[PS_NHAND][PS_NFINGER];
  double site_pos[PS_NHAND][PS_NFINGER][3];
  /* fixed tendons J0 = J2 + J1 (two dofs each) */
  int32_t tendon_dof[PS_NHAND][PS_HAND_NTENDON][2];
  double tendon_coef[PS_NHAND][PS_HAND_NTENDON][2];
  /* position actuators: target = dof (kind 0) or tendon (kind 1) */
  int32_t act_kind[PS_NHAND][PS_HAND_NACT];
  int32_t act_target[PS_NHAND][PS_HAND_NACT];
  double act_kp[PS_NHAND][PS_HAND_NACT];
  double act_ctrlrange[PS_NHAND][PS_HAND_NACT][2];
  int32_t act_forcelimited[PS_NHAND][PS_HAND_NACT];
  double act_forcerange[PS_NHAND][PS_HAND_NACT][2];
  /* capsule-capsule candidate pairs (global geom index = hand*PS_HAND_NGEOM + g),
   * after MuJoCo's filtering (same body, parent-child, <exclude>) */
  int32_t n_cappairs;
  int32_t cappair[PS_MAX_CAPPAIRS][2];
  /* mj_setConst-style inverse weights at qpos0 (regulariser scale diagApprox of the soft
   * constraints): translational body mobility trace(Jp M^-1 Jp^T)/3 and diag(M^-1). */
  double key_body_invweight[PS_NKEY];
  double key_dof_invweight[PS_NKEY];
  double body_invweight[PS_NHAND][PS_HAND_NBODY];
  double dof_invweight[PS_NHAND][PS_HAND_NDOF];
  /* extra colliders (type PS_GEOM_NONE = unused slot). Frame in the body frame; box: half
   * sizes; hull: vertices [xgeom_vert[0], +xgeom_vert[1]) of hull_vert in the geom frame,
   * whose origin is the hull's centre (MuJoCo's mesh frame). rbound: bounding-sphere radius
   * about the geom origin. Global collider ids: capsule h*PS_HAND_NGEOM + g, extra
   * PS_NHAND*PS_HAND_NGEOM + h*PS_HAND_NXGEOM + i. */
  int32_t xgeom_type[PS_NHAND][PS_HAND_NXGEOM];
  int32_t xgeom_body[PS_NHAND][PS_HAND_NXGEOM];
  double xgeom_pos[PS_NHAND][PS_HAND_NXGEOM][3];
  double xgeom_quat[PS_NHAND][PS_HAND_NXGEOM][4];
  double xgeom_size[PS_NHAND][PS_HAND_NXGEOM][3];
  double xgeom_rbound[PS_NHAND][PS_HAND_NXGEOM];
  int32_t xgeom_vert[PS_NHAND][PS_HAND_NXGEOM][2];
  double hull_vert[PS_NHAND][PS_HAND_HULLVERT][3];
  /* hand-hand candidate pairs with at least one extra collider (a < b, global ids), after
   * MuJoCo's filtering; contacts of these follow the capsule-capsule ones */
  int32_t n_xpairs;
  int32_t xpair[PS_MAX_XPAIRS][2];
  /* joint friction loss (MuJoCo dof_frictionloss; the Menagerie hand's right_hand class sets
   * 0.01 on every joint): each dof with frictionloss > 0 adds one friction-loss constraint row
   * J = e_dof, |f| <= frictionloss, to every substep's constraint solve, with the reference
   * acceleration -b (J v) and regulariser from solreffriction / solimpfriction (MuJoCo's
   * defaults (0.02, 1) and (0.9, 0.95, 0.001, 0.5, 2) unless the XML sets them). */
  double dof_frictionloss[PS_NHAND][PS_HAND_NDOF];
  double friction_solref[2], friction_solimp[5];
  /* MuJoCo body gravcomp of every hand body (PianoTask(gravity_compensation=True),
   * tasks/base.py:185-186: mujoco_utils.physics_utils.compensate_gravity sets 1): a passive force
   * -gravcomp m g at each hand body's COM, i.e. the hands feel (1 - gravcomp) of the gravity */
  double hand_gravcomp;
  /* Joints the reference's hand does not have - PianoTask(reduced_action_space=True) removes
   * THJ5, THJ1 and LFJ5 (shadow_hand.py:73-79,164-183), forearm_dofs without forearm_tx /
   * forearm_ty leaves that slide out (shadow_hand.py:270-311): the dof slot stays in qpos / qvel,
   * held at 0 with no force, no constraint row and no Jacobian entry, so its child body rides its
   * parent rigidly at the joint's zero - MuJoCo's body without that joint. */
  int32_t dof_locked[PS_NHAND][PS_HAND_NDOF];
  int32_t n_obs_joints[PS_NHAND];  /* joints_pos entries: dof_obs_order[h][0 .. n) (0: PS_HAND_NDOF) */
  /* The caller's action row: n_action columns, the last one the sustain pedal; act_column[h][a]
   * = actuator a's column, -1 when the reference has no such actuator (no force). n_action = 0:
   * the full PS_NACTION layout (actuator h * PS_HAND_NACT + a in that column). */
  int32_t act_column[PS_NHAND][PS_HAND_NACT];
  int32_t n_action;
} ps_model_desc;

/* Song tables: NoteTrajectory in dense form (music.py:SongTables). */
typedef struct {
  int32_t T;
  const float* goal;       /* [T][89]: keys + sustain */
  const int32_t* count;    /* [T] */
  const int32_t* keys;     /* [T][PS_MAX_NOTES] */
  const int32_t* fingers;  /* [T][PS_MAX_NOTES], 0-4 right, 5-9 left */
} ps_song_desc;

/* Task options (piano_with_shadow_hands.py:50-66). The first field is the struct's size: a
 * caller sets struct_size = sizeof(ps_task_cfg) (= PS_TASK_CFG_SIZE of the header it was built
 * against) and ps_create / ps_obs_dim refuse any other value - a caller built against an older
 * header (before ps_version 4: no struct_size, no solver_refine; before 5: no hand_side) fails with "rebuild against
 * include/pianosim.h" instead of the library reading past the end of its struct. */
typedef struct {
  uint32_t struct_size;             /* sizeof(ps_task_cfg) */
  int32_t n_steps_lookahead;        /* goal rows = lookahead + 1 */
  int32_t fingering_reward;         /* 1: fingering reward + 'fingering' obs; 0: OT reward */
  int32_t forearm_reward;           /* 1: add forearm reward term */
  int32_t wrong_press_termination;
  double energy_penalty_coef;       /* 5e-3 */
  int32_t solver_iterations;        /* Newton iterations per substep at most (0: the default cap, 24);
                                       reaching it is counted (PS_STAT_ITER_CAP) */
  int32_t max_contacts;             /* per env, <= PS_MAX_CONTACTS_LIMIT */
  int32_t canonical_actions;        /* 1: ps_step actions are in [-1,1] and are rescaled to the
                                       spec as dm_env_wrappers.CanonicalSpecWrapper does */
  int32_t solver;                   /* PS_SOLVER_NEWTON (the only value) */
  int32_t randomize_hand_positions; /* piano_with_shadow_hands.py:64,491-499: each episode shifts
                                       both hands by the same U(-0.05, 0.05) m along y */
  int32_t solver_refine;            /* 0: the Newton solve ends when its line search ends in the
                                       Hessian's piece; 1 (TaskConfig's default since round 6): then
                                       one more (refining) Newton step in that piece on the substeps
                                       whose hands are coupled, 2: on every substep - the fp32 solve's
                                       error shrinks (teacher-forced qpos p99 against the fp64 checker
                                       ~1.5e-4 -> ~8e-5 on coupled states) at ~5% of the throughput
                                       (DESIGN.md section 5). A solve that ends in the previous
                                       substep's guessed piece (one checked step) is not refined. */
  int32_t hand_side;                /* PS_HAND_BOTH: PianoWithShadowHands. PS_HAND_RIGHT / PS_HAND_LEFT:
                                       PianoWithOneShadowHand (piano_with_one_shadow_hand.py) with that
                                       hand; the model's other hand must be detached (every dof locked,
                                       no collider, no pair, no actuator: model.build_model(hand_side=)).
                                       Observation row: goal, fingering (5 wide, the kept hand's fingers,
                                       only with fingering_reward), piano/state, sustain, the kept hand's
                                       joints_pos, then the world position of its root (forearm) body, 3.
                                       Rewards: key_press, sustain, energy over the kept hand's actuators
                                       and, with fingering_reward, the fingering term over the kept hand's
                                       fingered notes (0 with none); no OT term (slot 3 is 0 without
                                       fingering_reward) and no forearm term (forearm_reward is ignored).
                                       randomize_hand_positions is refused. ps_fingertips keeps its shape:
                                       the detached hand's rows are its rest pose and mean nothing. */
  uint32_t observables;             /* PS_OBS_* bits (ps_version 7; 0: none): observables of the reference's
                                       entities that its task leaves disabled, appended to every env's
                                       row after the default part above, which keeps its width and bytes.
                                       Fixed order, whatever the bits' order of request:
                                       piano/joints_pos 88 (raw key angles), piano/activation 88 (0/1),
                                       piano/sustain_activation 1 (0/1); then for the right hand and then
                                       the left (hand_side: the kept hand only) joints_pos_cos_sin 2 nj
                                       (all cosines, then all sines), joints_vel nj, actuators_force na,
                                       actuators_velocity na, actuators_power na, fingertip_positions 15
                                       (th ff mf rf lf x xyz, world) and position 3 (the root body; the
                                       two-hand task only: the one-hand row has it already, the bit adds
                                       nothing there). nj: the hand's joints_pos entries, in their order;
                                       na: its actuators with an action column, in column order.
                                       Positions and velocities are the control step's final state;
                                       actuators_force is the last substep's actuation force (from the
                                       state before that substep's integration, clipped to forcerange);
                                       actuators_velocity the transmission velocity at the final state,
                                       actuators_power |force| |velocity| of those two (the energy term is
                                       -coef x their sum). A reset row holds mj_forward at the reset
                                       state with ctrl 0: velocities and power 0, force
                                       clip(kp (clamp(0, ctrlrange) - length), forcerange). Bits outside
                                       PS_OBS_ALL are refused. The field takes what was tail padding:
                                       sizeof(ps_task_cfg) is unchanged, so a caller built against an
                                       older header must have zeroed its struct. */
} ps_task_cfg;
#define PS_TASK_CFG_SIZE ((uint32_t)sizeof(ps_task_cfg))

/* ps_task_cfg.observables (piano.py:286-316, hands/base.py:75-114, shadow_hand.py:390-434).
 * joints_torque and fingertip_force are not modelled (they need MuJoCo's post-constraint RNE
 * and the touch sensors' contact sums): there is no bit for them. */
#define PS_OBS_PIANO_JOINTS_POS (1u << 0)
#define PS_OBS_PIANO_ACTIVATION (1u << 1)
#define PS_OBS_PIANO_SUSTAIN_ACTIVATION (1u << 2)
#define PS_OBS_JOINTS_POS_COS_SIN (1u << 3)
#define PS_OBS_JOINTS_VEL (1u << 4)
#define PS_OBS_ACTUATORS_FORCE (1u << 5)
#define PS_OBS_ACTUATORS_VELOCITY (1u << 6)
#define PS_OBS_ACTUATORS_POWER (1u << 7)
#define PS_OBS_FINGERTIP_POSITIONS (1u << 8)
#define PS_OBS_POSITION (1u << 9)
#define PS_OBS_ALL ((1u << 10) - 1)

/* Constraint solver. NEWTON (= EXACT, the only one): the minimiser of MuJoCo's primal
 * constraint problem over the accelerations (mj_solNewton: Newton directions from the
 * Hessian M + sum D J'J of the rows in their quadratic zone, exact line search), to fp32
 * (kernel) / 1e-13 (oracle) precision - the unique solution every MuJoCo solver converges
 * to. The round-1 truncated PGS (value 0) is retired; ps_create rejects it. */
#define PS_SOLVER_EXACT 1
#define PS_SOLVER_NEWTON 1
#define PS_HAND_BOTH 0
#define PS_HAND_RIGHT 1
#define PS_HAND_LEFT 2
#define PS_HAND_POSITION_OFFSET 0.05  /* piano_with_shadow_hands.py:46 _POSITION_OFFSET */

#define PS_MAX_CONTACTS_LIMIT 24
/* Constraint rows are not capped: friction loss (one per hand dof with frictionloss), hand and
 * key limits, 4 pyramid edges per contact. */

/* Physics warnings (MuJoCo mjWARN_BADQPOS / BADQVEL / BADQACC): mj_checkPos / mj_checkVel at
 * the start of a substep and mj_checkAcc after its constraint solve find a non-finite value or
 * one beyond 1e10 in qpos / qvel / qacc; the env's physics is reset as mj_resetData does (qpos
 * = qpos0, qvel = qacc_warmstart = ctrl = qfrc_applied = 0; after a bad qacc the forward
 * dynamics is recomputed at the reset state) and the warning is counted (ps_warnings). */
#define PS_WARN_BADQPOS 0
#define PS_WARN_BADQVEL 1
#define PS_WARN_BADQACC 2
#define PS_NWARN 3

/* step_type values (dm_env.StepType) */
#define PS_FIRST 0
#define PS_MID 1
#define PS_LAST 2

/* Reward term slots of ps_reward_terms (CompositeReward insertion order). */
#define PS_TERM_KEY_PRESS 0
#define PS_TERM_SUSTAIN 1
#define PS_TERM_ENERGY 2
#define PS_TERM_FINGERING 3   /* fingering_reward or ot_fingering_reward */
#define PS_TERM_FOREARM 4
#define PS_NTERMS 5

/* Slots of ps_musical_metrics (MidiEvaluationWrapper.get_musical_metrics keys). */
#define PS_MUS_PRECISION 0
#define PS_MUS_RECALL 1
#define PS_MUS_F1 2
#define PS_MUS_SUSTAIN_PRECISION 3
#define PS_MUS_SUSTAIN_RECALL 4
#define PS_MUS_SUSTAIN_F1 5
#define PS_NMUSIC 6

/* Slots of ps_solver_stats: per env, over the substeps of its last step. */
#define PS_STAT_SOLVES 0        /* Newton iterations (Hessian factorizations), summed */
#define PS_STAT_CONTACT_CAP 1   /* substeps whose narrow phase found >= max_contacts contacts */
#define PS_STAT_ITER_CAP 2      /* substeps whose Newton solve stopped at its iteration cap */
#define PS_STAT_MAX_ROWS 3      /* most contact rows (4 pyramid edges per contact) of one
                                   substep; the solve's other rows - one friction-loss row per hand
                                   dof with frictionloss and the violated hand / key limits - are
                                   not counted here */
#define PS_STAT_COUPLED 4       /* substeps whose hands were coupled (hand-hand contact or a key
                                   touched by both hands): the C-block elimination after both
                                   hands' independent pivots */
#define PS_STAT_BAD_PIVOT 5     /* substeps with a non-positive Cholesky pivot (clamped) */
#define PS_STAT_MAX_CDOFS 6     /* most coupled ("C") dofs of both hands in one substep (the dofs
                                   the hand-hand rows act on; > 28 takes the whole-block solve) */
#define PS_NSTATS 7

typedef struct ps_env ps_env;

const char* ps_last_error(void);
int ps_version(void);
/* the full hand (n_obs_joints = PS_HAND_NDOF, PS_HAND_NACT actuators); with cfg->hand_side the
 * one-hand row: (L+1)*89 + (5 if fingering) + 88 + 1 + 26 + 3; then the extras of cfg->observables.
 * < 0 (and a message) for a struct of another size or unknown PS_OBS_* bits. */
int ps_obs_dim(const ps_task_cfg* cfg);
/* sizeof(ps_model_desc), for host-side layout checks. */
int ps_model_desc_size(void);

int ps_create(const ps_model_desc* model, const ps_song_desc* song, const ps_task_cfg* cfg,
              int n_envs, int device, uint64_t seed, ps_env** out);
void ps_destroy(ps_env* env);
/* The handle's observation width and action row width (the model's joints_pos entries and
 * actuators: the reference's VecEnv shapes, parallelized_base_v2.py:41-51); the width includes
 * the extras of ps_task_cfg.observables, sized by the model's joints_pos entries and actuators. */
int ps_env_obs_dim(const ps_env* env);
int ps_env_action_dim(const ps_env* env);

/* Resets envs (all when env_mask == NULL, else where env_mask[i] != 0; device u8[N])
 * and writes their first observation into obs[N][obs_dim]. */
int ps_reset(ps_env* env, const uint8_t* env_mask, float* obs, void* stream);

/* action[N][ps_env_action_dim] (45 for the full hand) in spec units, or canonical [-1,1] units
 * when cfg.canonical_actions. Envs whose
 * previous step was LAST are reset instead and report PS_FIRST (reward 0, discount 1). */
int ps_step(ps_env* env, const float* action, float* obs, float* reward, float* discount,
            uint8_t* step_type, void* stream);

/* qpos/qvel/qacc_warmstart [N][140] (MuJoCo dof order: keys, right hand, left hand),
 * ctrl [N][44], sustain [N], t_idx [N], last [N] (1 if the previous step was LAST). */
int ps_get_state(ps_env* env, float* qpos, float* qvel, float* qacc_ws, float* ctrl,
                 float* sustain, int32_t* t_idx, uint8_t* last, void* stream);
int ps_set_state(ps_env* env, const float* qpos, const float* qvel, const float* qacc_ws,
                 const float* ctrl, const float* sustain, const int32_t* t_idx,
                 const uint8_t* last, void* stream);
/* Generalized applied force [N][140] added every substep until changed (NULL clears). */
int ps_set_applied(ps_env* env, const float* qfrc_applied, void* stream);
/* Per-term rewards of the last step, [N][PS_NTERMS]. */
int ps_reward_terms(ps_env* env, float* terms, void* stream);
/* Fingertip site positions after the last step/reset, [N][2][5][3] (right, left). */
int ps_fingertips(ps_env* env, float* xpos, void* stream);
/* Number of contacts after the last step/reset, [N]. Without contact recording a step or reset
 * runs the final-state collision pass only for the envs whose forearm term needs it; the counts
 * are then computed here, by one launch of that pass over the state rows (as ps_set_state and
 * ps_set_hand_offset do before they overwrite what it reads). Captured into a graph, the call
 * always includes that launch. */
int ps_contact_count(ps_env* env, int32_t* ncon, void* stream);

/* One contact of the task layer's final collision pass (physics.data.contact after the step):
 * position (world), frame (normal geom1 -> geom2, two tangents), signed distance (< 0:
 * penetration), kind (0 hand-key, 1 hand-base, 2 hand-hand), key index (kind 0), global
 * collider ids g1 (-1 for a key or the base) and g2. */
typedef struct {
  float pos[3], n[3], t1[3], t2[3], dist;
  int32_t kind, key, g1, g2;
} ps_contact;
/* Contact lists of each env's last step: ps_record_contacts(env, 1) makes the step kernel
 * keep them (off by default: ~70 B per contact of extra HBM writes); ps_contacts copies them
 * to out [N][PS_MAX_CONTACTS_LIMIT] (device; the first ncon of each env are valid), in the
 * order capsule-piano, capsule-capsule, box / hull-piano, box / hull hand-hand (round 6; the
 * checker's, oracle/pianosim_ref.c collide). No reference counterpart beyond
 * physics.data.contact; used for collision parity checks. */
int ps_record_contacts(ps_env* env, int on);
int ps_contacts(ps_env* env, ps_contact* out, void* stream);

/* Musical metrics of each env's LAST finished episode, [N][PS_NMUSIC] (per-step binary
 * precision / recall / F1 with zero_division = 1, as sklearn's precision_recall_fscore_support
 * in evaluation.py:114-177, averaged over the episode's steps), and the number of episodes
 * each env has finished since ps_create, [N]. Device pointers; either may be NULL. */
int ps_musical_metrics(ps_env* env, float* episode, int32_t* episodes, void* stream);

/* Solver / cap counters of each env's last step, [N][PS_NSTATS] int32 (device). No reference
 * counterpart: the evidence that the contact and row caps do not bind. */
int ps_solver_stats(ps_env* env, int32_t* stats, void* stream);

/* Physics warnings of each env since ps_create, [N][PS_NWARN] int32 (device): the counts of
 * mj_checkPos / mj_checkVel / mj_checkAcc resets (see PS_WARN_*). dm_control turns a new
 * warning into PhysicsError (Physics.check_invalid_state); envs.Environment does the same. */
int ps_warnings(ps_env* env, int32_t* warnings, void* stream);

/* Episode-return bookkeeping of a rollout loop in one launch (the reference driver's per-env
 * return sums, parallelized_base_v2.py / ppo_v2.py training loops): after a step with rewards
 * reward[n] and step types step_type[n] (uint8), running[i] (f64) restarts at a FIRST step and
 * accumulates the reward otherwise; at a LAST step last_return[i] (f32) takes it and it is added
 * to *finished_sum (f64) and *finished_count (int64). Device pointers; no env handle. */
int ps_episode_returns(const float* reward, const uint8_t* step_type, int n, double* running, float* last_return,
                       double* finished_sum, int64_t* finished_count, void* stream);

/* randomize_hand_positions (piano_with_shadow_hands.py:491-499): each env's current y shift of
 * both hand roots [N] f32 and its resets so far [N] i32 (device; either may be NULL). The set
 * form overrides the shift until the env's next reset (teacher-forced parity). */
int ps_get_hand_offset(ps_env* env, float* dy, int32_t* episodes, void* stream);
int ps_set_hand_offset(ps_env* env, const float* dy, void* stream);

/* Global id of this handle's env 0 when the envs of one job are sharded over handles/GPUs
 * (default 0). Every per-env random draw (the randomize_hand_positions Philox stream) is keyed
 * by (seed, global env id, episode), so a global env draws the same values at any world size
 * ("Philox streams are keyed by global env id"). */
int ps_set_env_offset(ps_env* env, int64_t global_first_env);

/* ---- per-episode MIDI augmentations (PianoWithShadowHands(augmentations=...),
 * piano_with_shadow_hands.py:62,151-157,169-174, over the Variations of suite/variations.py:
 * MidiSelect, MidiTemporalStretch, MidiPitchShift, MidiOctaveShift). Every episode of every env,
 * the first reset included, starts again from the bank's song 0 (the song given to ps_create),
 * applies the variations in list order and plays the result. Which envs start an episode is
 * known on the device only (auto-reset after LAST), so the draw and the env's new song tables
 * are made there, by a builder kernel that ps_reset and ps_step enqueue before their own: no
 * host sync, legal under stream capture. The draw is counter-based (Philox4x32-10 keyed by the
 * handle's seed, counter (episode, global env id, "midi", index in the list)), not numpy's
 * RandomState stream; DESIGN.md states it and variations.draw restates it in Python.
 *
 * A song of the bank (host memory; copied): notes (pitch, start, end, part) as fp64, stably
 * sorted by start time, the CC64 events (time, value) in sequence order, total_time, one bit per
 * MIDI pitch that occurs (word p / 32, bit p % 32). Layout of pss_flat_song (pianosong.h),
 * whose pss_flatten writes it. A positive stretch factor keeps the order: the device never sorts. */
typedef struct {
  const double* notes;
  const double* ccs;
  int32_t n_notes, n_cc;
  double total_time;
  uint32_t pitch_mask[4];
} ps_aug_song;
#define PS_VAR_SELECT 1   /* one of songs 1 .. n_songs - 1, uniformly; no gate */
#define PS_VAR_STRETCH 2  /* factor uniform on [1 - range, 1 + range] */
#define PS_VAR_PITCH 3    /* semitones uniform on [max(21 - min_pitch, -range), min(108 - max_pitch, range)] */
#define PS_VAR_OCTAVE 4   /* 12 x uniform on [low // 12, high // 12] of the bounds at 12 * range */
#define PS_MAX_VARIATIONS 4
typedef struct {
  int32_t kind;
  double prob;  /* the variation is skipped when u > prob */
  double range; /* 0: no-op */
} ps_variation;
typedef struct {
  uint32_t struct_size;  /* sizeof(ps_augment_desc), as ps_task_cfg.struct_size */
  int32_t n_songs;
  const ps_aug_song* songs;
  int32_t n_variations;  /* <= PS_MAX_VARIATIONS */
  const ps_variation* variations;
  double dt, initial_buffer_time;  /* the control timestep and buffer the song of ps_create was built with */
  int32_t T_cap;       /* rows of one env's tables: the most frames any song takes at the largest
                          stretch factor, plus the buffer frames */
  uint64_t max_bytes;  /* budget of the per-env tables (n_envs * T_cap * 488 B); 0: none */
} ps_augment_desc;
#define PS_AUGMENT_DESC_SIZE ((uint32_t)sizeof(ps_augment_desc))
/* Init-time (it allocates and synchronises): call before the first reset. NULL turns the
 * augmentations off and frees the bank. Every env starts with the tables of song 0 as given.
 * Fails, with the sizes in the message, when the per-env tables exceed max_bytes, when a song
 * as given does not fit T_cap rows of at most PS_MAX_NOTES keys, or when the builder's roll
 * ((T_cap - buffer frames) * 89 B) does not fit the 64 KB of LDS a workgroup may take. */
int ps_set_augmentations(ps_env* env, const ps_augment_desc* desc);
/* This episode's draw of each env: song [N] i32 (index into the bank), factor [N] f64, shift [N]
 * i32 (semitones), its length T [N] i32, and fallbacks [N] i32: how often since
 * ps_set_augmentations a draw would have needed more than T_cap rows or put more than
 * PS_MAX_NOTES keys into one row - that episode then plays the selected song at factor 1.0 and
 * shift 0 (a truncated table is never written). Device pointers; any may be NULL. */
int ps_get_augmentation(ps_env* env, int32_t* song, double* factor, int32_t* shift, int32_t* T,
                        int32_t* fallbacks, void* stream);
/* Forces the draw of every env (device arrays [N]) and rebuilds its tables now; it holds until
 * the env's next reset, like ps_set_hand_offset (teacher-forced parity). */
int ps_set_augmentation(ps_env* env, const int32_t* song, const double* factor, const int32_t* shift,
                        void* stream);
/* The per-env tables: goal [N][T_cap][89] f32, count [N][T_cap], keys / fingers
 * [N][T_cap][PS_MAX_NOTES] i32 (device; any may be NULL); rows >= T of an env are stale. */
int ps_get_song_tables(ps_env* env, float* goal, int32_t* count, int32_t* keys, int32_t* fingers,
                       void* stream);

/* ---- the piano's sound module on the device (robopianist/models/piano/midi_module.py, driven
 * after every physics substep from piano.py:154-162): every env's NoteOn / NoteOff / SustainOn /
 * SustainOff messages, stamped with the substep they happened in. A recording handle's step
 * kernel keeps the key and sustain activations at the end of every substep, and a second kernel
 * that ps_step and ps_reset enqueue after it appends what changed to the env's running episode:
 * no host sync, legal under stream capture. Inside one substep the order is the reference's:
 * NoteOns by ascending key, NoteOffs by ascending key, SustainOn, SustainOff.
 *
 * An event is one uint32: bits 0-7 the MIDI note number (key + 21; 0 for the pedal), bits 8-9
 * the kind (PS_MIDI_*), bits 10-31 the substep's ordinal in the episode, the first substep
 * being 1. Its time is ordinal * timestep: physics.data.time after that substep. The velocity is
 * the reference's constant 127. After a physics warning (PS_WARN_*) MuJoCo's time restarts at 0;
 * the ordinal goes on, and the keys' jump to 0 gives their NoteOffs.
 *
 * Per env two banks of max_events events: the running episode and the last finished one (a
 * reset, ps_reset's or the auto-reset after LAST, swaps them), so a finished performance stays
 * readable for the whole next episode. An event that does not fit is counted in `dropped` and
 * not written. */
#define PS_MIDI_NOTE_ON 0
#define PS_MIDI_NOTE_OFF 1
#define PS_MIDI_SUSTAIN_ON 2
#define PS_MIDI_SUSTAIN_OFF 3
#define PS_MIDI_ORDINAL_SHIFT 10
#define PS_MIDI_ORDINAL_MAX ((1u << 22) - 1) /* later substeps keep this ordinal */
/* Init-time (it allocates and synchronises; not under stream capture): turns recording on with
 * banks of max_events events, or off (max_events 0), freeing the buffers. Recording starts with
 * all keys and the pedal taken as off. n_envs * (8 * max_events + 4 * (1 + 3 * n_substeps) + 40)
 * bytes; fails, with the sizes in the message, when that exceeds max_bytes (0: no limit) - the
 * handle is then left as it was, recording or not. Every other call replaces the banks: what
 * was recorded before it is gone. */
int ps_record_midi(ps_env* env, int max_events, uint64_t max_bytes);
/* Bank `which` (0: the running episode, 1: the last finished one) of every env: events
 * [N][max_events] (the first count[i] of env i are valid), count / dropped [N], substeps [N] (the
 * episode's physics substeps so far: its length is substeps * timestep). Device pointers; any
 * may be NULL. */
int ps_midi_events(ps_env* env, int which, uint32_t* events, int32_t* count, int32_t* dropped,
                   int32_t* substeps, void* stream);
/* MidiModule.after_substep as an entry point: appends the messages of caller-supplied activation
 * rows bits [N][rows][3] (device) to every env's running episode, as if a step had produced them:
 * key k is bit k % 32 of word k / 32, the sustain activation bit 24 of word 2; 1 <= rows <= the
 * handle's n_substeps. */
int ps_midi_push(ps_env* env, const uint32_t* bits, int rows, void* stream);

/* ---- snapshots (ps_version 8): save, restore and fork whole envs on the device.
 *
 * A snapshot holds one row per env of every per-env device buffer of the handle that a later
 * step, reset or getter reads: the dynamic state (qpos, qvel, qacc_ws, ctrl, sustain, t_idx,
 * last), qfrc_applied, the last step's outputs kept for the getters (reward terms, fingertips,
 * contact counts, solver stats, warnings), the musical-metric accumulators, the hand offset and
 * the episode counter; on an augmented handle the env's draw and its own song tables; with
 * contact recording on its contact list; with the MIDI recorder on its two event banks, the
 * recorder's words and the capture row's header. The step kernels' scratch (the parked lane
 * state, the queue and the dispatch order) is rewritten by every step before it is read and is
 * not saved. The caller-owned obs / reward / discount / step_type buffers are the caller's to
 * keep.
 *
 * The rows are listed once, at create time; save and restore walk that one list. A snapshot
 * belongs to the handle it was created on and to that handle's configuration at the time:
 * ps_set_augmentations, ps_record_midi or ps_record_contacts after the create change the list,
 * and save / restore then fail (with a message, launching nothing), as they do on another handle.
 *
 * ps_snapshot_create allocates n_envs * (the sum of the row sizes, each rounded up to 16 B)
 * bytes and fails, with the sizes in the message, when that exceeds max_bytes (0: no limit): an
 * augmented handle's tables are 488 B per env and row. It saves nothing yet. Init-time.
 *
 * ps_snapshot_save first makes the lazy contact counts real (as ps_set_state does), then copies
 * every row. ps_snapshot_restore is one kernel launch. src == NULL: every env takes its own row.
 * src [N] (device): env i takes the row of env src[i] - the fork. src[i] == -1 leaves env i as
 * it is; any other index outside [0, N) leaves it as it is too and adds one to *n_bad (device,
 * may be NULL; the caller zeroes it). Both are asynchronous on the stream and legal under
 * stream capture.
 *
 * The per-env random draws (randomize_hand_positions, the augmentations) stay keyed by (seed,
 * global env id, episode). A fork copies the source's episode counter, but the destination keeps
 * its own id: forks of one env are bitwise copies until their next reset and draw different
 * hand offsets / augmentations there. That is intended - a fork is another env at the same
 * state, not a replay; ps_snapshot_restore with src == NULL is the replay. */
typedef struct ps_snapshot ps_snapshot;
int ps_snapshot_create(ps_env* env, uint64_t max_bytes, ps_snapshot** out);
uint64_t ps_snapshot_bytes(const ps_snapshot* snap);
int ps_snapshot_save(ps_env* env, ps_snapshot* snap, void* stream);
int ps_snapshot_restore(ps_env* env, const ps_snapshot* snap, const int32_t* src, int32_t* n_bad, void* stream);
void ps_snapshot_destroy(ps_snapshot* snap);

/* ---- rendering (ps_version 9): ray-cast cameras over the envs' analytic scene
 * (physics.render(height, width, camera_id, depth, segmentation); the named cameras of
 * models/piano/piano.py:100-141 are restated in rendering.py).
 *
 * The scene of an env is a function of its qpos row, its hand offset and (for the key colours) its
 * t_idx and song tables: the hands' capsule, box and convex-hull colliders, the 88 key boxes each
 * rotated about its hinge, the base box and a floor, the plane z = 0 (visual only, as the
 * reference's stage). Unused collider slots, and with them the detached hand of the one-hand
 * task, are not drawn. No meshes, textures, shadows, transparency or anti-aliasing.
 *
 * Camera: position, image right x and image up y (orthonormalised by the call, x first), vertical
 * field of view in degrees; it looks along -z = -(x cross y). Row 0 of an image is its top. The
 * ray of pixel (r, c) of an H x W image goes through the pixel's centre:
 *   d = px x + py y - z,  py = (1 - 2 (r + 1/2) / H) tan(fovy / 2),
 *                         px = (2 (c + 1/2) / W - 1) tan(fovy / 2) W / H.
 * d is not normalised, so the parameter t of the first hit pos + t d is the depth along the
 * optical axis (dm_control's depth). Only entering hits with t > 0 count (a camera inside an
 * object does not see it); of two objects at the same t the lower id is drawn. A miss: depth +inf,
 * segmentation -1, the background colour.
 *
 * Segmentation ids: global collider id g (capsule h * PS_HAND_NGEOM + i, then extra collider
 * PS_NHAND * PS_HAND_NGEOM + h * PS_HAND_NXGEOM + i) 0 .. 63, key k PS_SEG_KEY0 + k, the base
 * PS_SEG_BASE, the floor PS_SEG_FLOOR.
 *
 * Shading: a headlight at the camera. With n the unit outward normal at the hit and dhat = d / |d|,
 *   rgb[k] = floor(255 clamp(colour[k] (PS_RENDER_AMBIENT + PS_RENDER_DIFFUSE max(0, -n . dhat)), 0, 1) + 1/2);
 * a miss is the background colour unshaded. Colours (PS_RENDER_COLOR_*; piano_constants.py:83-85,
 * piano.py:28, shadow_hand_constants.py:42-49): white key 0.9, black key 0.1, base 0.15, activated
 * key (0.2, 0.8, 0.2), fingers th ff mf rf lf (0.8, 0.2, 0.8) (0.8, 0.2, 0.2) (0.2, 0.8, 0.8)
 * (0.2, 0.2, 0.8) (0.8, 0.8, 0.2), hand 0.6, floor (0.2, 0.3, 0.4), background (0.05, 0.05, 0.1).
 * PS_RENDER_ACTIVATION (change_color_on_activation): a key at activation (the task's rule:
 * |clip(q, range) - range max| <= 0.5 degrees) takes the activation colour.
 * PS_RENDER_COLORIZE (_colorize_fingertips / _colorize_keys): the colliders on a fingertip site's
 * body (the distal links) take their finger's colour, and a key in the goal row of the step just
 * played (row t_idx - 1; none right after a reset) that is not activated takes the colour of the
 * finger the song tables assign to it (none for a song without fingering; the one-hand task: its
 * hand's notes only).
 * PS_RENDER_COUNT_LIST (diagnostic): every tile adds its culled list's length to a counter that
 * ps_render_list_stats reads. */
typedef struct {
  double pos[3];
  double x[3], y[3];
  double fovy_deg;
} ps_camera;
#define PS_RENDER_ACTIVATION (1u << 0)
#define PS_RENDER_COLORIZE (1u << 1)
#define PS_RENDER_COUNT_LIST (1u << 16)
#define PS_RENDER_ALL (PS_RENDER_ACTIVATION | PS_RENDER_COLORIZE | PS_RENDER_COUNT_LIST)
#define PS_SEG_KEY0 64
#define PS_SEG_BASE 152
#define PS_SEG_FLOOR 153
#define PS_RENDER_AMBIENT 0.3f
#define PS_RENDER_DIFFUSE 0.7f
#define PS_RENDER_COLOR_WHITE 0
#define PS_RENDER_COLOR_BLACK 1
#define PS_RENDER_COLOR_BASE 2
#define PS_RENDER_COLOR_ACTIVATION 3
#define PS_RENDER_COLOR_FINGER0 4 /* + finger: th ff mf rf lf */
#define PS_RENDER_COLOR_HAND 9
#define PS_RENDER_COLOR_FLOOR 10
#define PS_RENDER_COLOR_BACKGROUND 11
#define PS_RENDER_NCOLOR 12
/* Renders the envs envs[0 .. n_sel) (device int32; repeats and any order allowed; NULL: all N envs
 * in order, n_sel = N) through one camera into rgb u8 [n_sel][height][width][3], depth f32
 * [n_sel][height][width] and seg i32 [n_sel][height][width] (device; any may be NULL, not all). An
 * index outside [0, N) leaves its image untouched and adds one to *n_bad (device, may be NULL; the
 * caller zeroes it). Asynchronous on the stream: a render after a step sees that step. It reads
 * env memory and writes its outputs and a scratch of the handle (9792 B per selected env, grown to
 * the largest n_sel so far) only. A handle's first call builds the hulls' face planes on the host
 * (at most 96 per hull, else an error naming the hull) and allocates: init-time, not under stream
 * capture; handles that never render allocate nothing. Refused with an error: width, height or
 * n_sel <= 0, fovy outside (0, 180), a zero x or a y that is zero or parallel to x, all three
 * outputs NULL, unknown flag bits. */
int ps_render(ps_env* env, const ps_camera* cam, int width, int height, const int32_t* envs, int n_sel,
              uint32_t flags, uint8_t* rgb, float* depth, int32_t* seg, int32_t* n_bad, void* stream);
/* PS_RENDER_COUNT_LIST's counter (host memory; it synchronises): sum_tiles[0] the summed list
 * lengths, [1] the tiles counted; reset != 0 zeroes it afterwards. */
int ps_render_list_stats(ps_env* env, uint64_t* sum_tiles, int reset);

#ifdef __cplusplus
}
#endif
#endif
