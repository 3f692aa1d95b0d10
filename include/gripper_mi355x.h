/* gripper_mi355x.h -- C ABI of the MI355X-native batched gripper env-step path.
 *
 * This is the drop-in boundary that replaces the per-env MjClass hot path which
 * the reference exposes through pybind11 (src/bind.cpp:32-205, compiled to
 * rl/env/mjpy/bind.so by Makefile:22,31,155-156).  Every entry point below names
 * the reference interface it replaces.  Conventions:
 *   - plain C types and pointers only; no C++ exceptions cross the ABI;
 *   - every call returns GM_OK (0) or a negative GM_E* code, and the per-context
 *     message is available from gm_last_error(ctx) (the Python facade raises
 *     RuntimeError with it, as pybind11's default translator does for
 *     std::runtime_error in the reference);
 *   - host buffers are owned by the caller; `on_device != 0` means the pointer is
 *     a HIP device pointer on the context's device (zero-copy torch tensors);
 *   - one context per HIP stream; calls on one context are not reentrant.
 *
 * The interface data types (settings, model, object descriptors) are plain POD
 * structs; tests/ hand the same structs to the CPU oracle in oracle/.
 */
#ifndef GRIPPER_MI355X_H_
#define GRIPPER_MI355X_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ limits */
#define GM_MAX_SEG    10      /* finger segment joints N (reference: 5..10)   */
#define GM_MAX_BODY   40
#define GM_MAX_DOF    44      /* 3 (N + 2) + 8 for N = 10                    */
#define GM_MAX_QPOS   48
#define GM_MAX_GEOM   40
#define GM_MAX_PAIR   80      /* 6 N + 15 candidate pairs; a lane per pair per 64-pair batch */
#define GM_MAX_CON    32      /* contacts kept per env per substep (box-box: up to 8 per pair) */
#define GM_MAX_EFC    (4 * GM_MAX_CON + GM_MAX_LOCK)   /* rows: motor locks + 4 pyramid edges per contact */
#define GM_NEWTON_MAXIT 16    /* Newton iterations per substep (cap; converged runs stop earlier) */
#define GM_NEWTON_MAXLS 16    /* exact line-search evaluations per Newton iteration (cap)          */
#define GM_MAX_LOCK   4       /* prismatic x3 + palm (revolute locks disabled) */
#define GM_MAX_OBJSET 64      /* objects in one synthetic object set          */
#define GM_RING       64      /* sensor window: last 64 readings per stream (1 + rps * prev_steps <= 64) */
#define GM_CHAIN      (GM_MAX_SEG + 2)  /* dofs per finger chain below base   */
/* MPR support-point tie band: a unit direction whose body-frame component along a box
 * face normal / cylinder axis is below this picks the face centre (see support_geom) */
#define GM_SUPPORT_TIE 1e-9

/* ------------------------------------------------------------------ errors */
#define GM_OK            0
#define GM_E_ARG        -1
#define GM_E_HIP        -2
#define GM_E_STATE      -3
#define GM_E_NOEXT      -4
#define GM_E_RANGE      -5

/* ------------------------------------------------------------- geom types */
/* numbering follows MuJoCo's mjtGeom so the (geom1, geom2) canonical order
 * "lower type first, then lower id" is the one the reference's contact signs
 * depend on (hard part 3). */
#define GM_GEOM_PLANE    0
#define GM_GEOM_SPHERE   2
#define GM_GEOM_CAPSULE  3
#define GM_GEOM_CYLINDER 5
#define GM_GEOM_BOX      6

/* contact classes: Contact::check_involves() prefixes (objecthandler.h:117-129) */
#define GM_CLS_NONE    0
#define GM_CLS_FINGER1 1
#define GM_CLS_FINGER2 2
#define GM_CLS_FINGER3 3
#define GM_CLS_PALM    4
#define GM_CLS_GROUND  5
#define GM_CLS_OBJECT  6

/* joint types (MuJoCo mjtJoint numbering) */
#define GM_JNT_FREE   0
#define GM_JNT_SLIDE  2
#define GM_JNT_HINGE  3

/* body chain groups: which compact Jacobian block a body's dofs live in */
#define GM_GRP_WORLD  -1
#define GM_GRP_FINGER0 0
#define GM_GRP_PALM    3
#define GM_GRP_BASE    4
#define GM_GRP_OBJECT  5

/* ------------------------------------------------------------ settings */
typedef struct gm_sensor {            /* MjType::Sensor, mjclass.h:79-241 */
  int32_t in_use;
  float   normalise;
  float   read_rate;
  int32_t use_normalisation;
  int32_t use_noise;
  float   raw_value_offset;
  float   noise_mag;
  float   noise_mu;
  float   noise_std;
  int32_t noise_overriden;
  int32_t prev_steps;
  int32_t readings_per_step;
  int32_t total_readings;
} gm_sensor;

typedef struct gm_action {            /* MjType::ActionSetting, mjclass.h:458-572 */
  int32_t in_use;
  int32_t continous;
  double  value;
  int32_t sign;
} gm_action;

typedef struct gm_binary_reward {     /* MjType::BinaryReward, mjclass.h:649-663 */
  float   reward;
  int32_t done;
  int32_t trigger;
} gm_binary_reward;

typedef struct gm_linear_reward {     /* MjType::LinearReward, mjclass.h:665-684 */
  float   reward;
  int32_t done;
  int32_t trigger;
  float   min;
  float   max;
  float   overshoot;
} gm_linear_reward;

typedef struct gm_settings {          /* MjType::Settings, mjclass.h:736-779 */
#define GM_XX(n, t, v) t n;
#define GM_SS(n, u, nm, r) gm_sensor n;
#define GM_AA(n, u, v, s) gm_action n;
#define GM_BR(n, r, d, t) gm_binary_reward n;
#define GM_LR(n, r, d, t, a, b, o) gm_linear_reward n;
#include "gm_settings.def"
} gm_settings;

/* event indices, in settings order (binary first, then linear) */
enum {
#define GM_BR(n, r, d, t) GM_EV_##n,
#include "gm_settings.def"
  GM_N_BINARY
};
enum {
#define GM_LR(n, r, d, t, a, b, o) GM_LEV_##n,
#include "gm_settings.def"
  GM_N_LINEAR
};
enum {
#define GM_AA(n, u, v, s) GM_ACT_##n,
#include "gm_settings.def"
  GM_N_ACTION_KINDS
};
/* action codes, MjType::Action (mjclass.h:40-63): 3 per action kind + termination */
#define GM_ACTION_CODE_COUNT (3 * GM_N_ACTION_KINDS + 1)
#define GM_ACTION_TERMINATION (3 * GM_N_ACTION_KINDS)

/* sample modes, MjType::Sample (mjclass.h:66-76) */
#define GM_SAMPLE_RAW 0
#define GM_SAMPLE_CHANGE 1
#define GM_SAMPLE_AVERAGE 2
#define GM_SAMPLE_MEDIAN 3
#define GM_SAMPLE_SIGN 4
#define GM_SAMPLE_SCALED_CHANGE 5
#define GM_SAMPLE_SCALED_CHANGE_SQ 6

/* Derived configuration: what MjClass::configure_settings() (mjclass.cpp:97-314)
 * and Settings::update_sensor_settings() (mjclass.cpp:5236-5265) compute from
 * gm_settings.  Built on the host by gm_configure(); shared by all envs. */
typedef struct gm_config {
  gm_settings s;
  int32_t n_actions;
  int32_t action_options[GM_ACTION_CODE_COUNT];
  int32_t sensor_fcn;                 /* sample mode for sensors            */
  int32_t state_fcn;                  /* sample mode for state sensors      */
  int32_t sensor_fcn_state_override;  /* reference quirk mjclass.cpp:204-206 */
  int32_t sim_steps_per_action;
  int32_t n_obs;
  double  timestep;
  double  sim_gauge_raw_to_N_factor;  /* mjclass.cpp:281                    */
  double  base_min[6];                /* x,y,z,roll,pitch,yaw (myfunctions.cpp:245-261) */
  double  base_max[6];
} gm_config;

/* ------------------------------------------------------------ model */
typedef struct gm_model_params {      /* numerics the MJCF would carry (myfunctions.cpp:836-953) */
  int32_t n_seg;                      /* N finger segment joints              */
  double  finger_length;              /* 235e-3                               */
  double  finger_width;               /* 28e-3                                */
  double  finger_thickness;           /* 0.86e-3 (baseline yaml)              */
  double  finger_E;                   /* 193e9                                */
  double  hook_length;                /* 35e-3                                */
  double  hook_angle_degrees;         /* 75                                   */
  double  fingertip_clearance;        /* 10e-3                                */
  double  segment_inertia_scaling;    /* 50                                   */
  double  timestep;                   /* 3.187e-3 (test.cpp:207)              */
  int32_t pgs_iterations;             /* sweeps of the oracle's PGS cross-check */
  double  collision_half_thickness;   /* finger plate collision half-thickness */
  /* segment hinge damping d = segment_damping * N^-segment_damping_power and armature
   * a = segment_armature * N^-segment_armature_power (absent from the reference sources:
   * fitted to its measured stable timesteps, tests/test_calibration.py) */
  double  segment_damping;
  double  segment_damping_power;
  double  segment_armature;
  double  segment_armature_power;
  /* actuators (the reference writes ctrl to MJCF motors, luke::control myfunctions.cpp:1912-2057):
   * 1 = MuJoCo 2.1.5's order -- the PD forces explicit between mj_step1 and mj_step2, the
   * constraint solve on M + armature, joint damping implicit in mj_Euler; 0 = the PD gains
   * and joint damping folded implicitly into the solve's matrix (rounds 1-3) */
  int32_t mujoco_actuators;
  int32_t pad_params;
  /* armature of the actuated joints (prismatic, revolute, palm, base): the motors'
   * reflected inertia the absent MJCF would carry (invented; DESIGN.md "Model spec") */
  double  actuator_armature[4];
} gm_model_params;

typedef struct gm_model {
  int32_t nbody, njnt, nq, nv, ngeom, npair, nlock, n_seg;
  /* bodies (parent always has a lower index) */
  int32_t body_parent[GM_MAX_BODY];
  int32_t body_jnt[GM_MAX_BODY];      /* -1 = welded to parent             */
  int32_t body_group[GM_MAX_BODY];    /* GM_GRP_*                          */
  double  body_pos[GM_MAX_BODY][3];   /* in parent frame                   */
  double  body_quat[GM_MAX_BODY][4];  /* w,x,y,z in parent frame           */
  double  body_mass[GM_MAX_BODY];
  double  body_ipos[GM_MAX_BODY][3];  /* centre of mass, body frame        */
  double  body_inertia[GM_MAX_BODY][3]; /* principal, body-frame aligned   */
  /* joints: at most one per body */
  int32_t jnt_type[GM_MAX_BODY];
  int32_t jnt_body[GM_MAX_BODY];
  int32_t jnt_qposadr[GM_MAX_BODY];
  int32_t jnt_dofadr[GM_MAX_BODY];
  double  jnt_pos[GM_MAX_BODY][3];    /* anchor, body frame                */
  double  jnt_axis[GM_MAX_BODY][3];   /* body frame, unit                  */
  double  jnt_stiffness[GM_MAX_BODY];
  double  jnt_damping[GM_MAX_BODY];
  double  jnt_armature[GM_MAX_BODY];
  /* dofs */
  int32_t dof_parent[GM_MAX_DOF];
  int32_t dof_body[GM_MAX_DOF];
  int32_t dof_group[GM_MAX_DOF];      /* GM_GRP_* of the owning chain       */
  int32_t dof_slot[GM_MAX_DOF];       /* index inside the compact group block */
  /* geoms */
  int32_t geom_type[GM_MAX_GEOM];
  int32_t geom_body[GM_MAX_GEOM];
  int32_t geom_class[GM_MAX_GEOM];
  double  geom_pos[GM_MAX_GEOM][3];
  double  geom_quat[GM_MAX_GEOM][4];
  double  geom_size[GM_MAX_GEOM][3];
  double  geom_friction[GM_MAX_GEOM];
  double  geom_rbound[GM_MAX_GEOM];
  /* candidate pairs (object pairs first; unordered: canonical order per env) */
  int32_t pair_a[GM_MAX_PAIR];
  int32_t pair_b[GM_MAX_PAIR];
  /* motor locks (reference weld constraints on 1-DoF motors) */
  int32_t lock_dof[GM_MAX_LOCK];
  int32_t lock_kind[GM_MAX_LOCK];     /* 0 prismatic, 2 palm               */
  /* keyframe "initial pose" (myfunctions.cpp:171) */
  double  qpos0[GM_MAX_QPOS];
  /* mj_setConst at qpos0: body_invweight0 (translation, rotation: the mean diagonal of
   * J M^-1 J^T at the body's centre of mass) and dof_invweight0 (M^-1 diagonal); they set
   * the constraint regulariser R = (1 - d) / d * diagApprox (mj_diagApprox).  Derived by
   * gm_build_model / gm_model_from_mjcf; the live object's are per env. */
  double  body_invweight0[GM_MAX_BODY][2];
  double  dof_invweight0[GM_MAX_DOF];
  /* named indices */
  int32_t dof_base, dof_palm, dof_obj;
  int32_t dof_pris[3], dof_rev[3], dof_seg[3];   /* first segment dof per finger */
  int32_t body_base, body_finger[3], body_palm, body_obj, geom_obj, geom_ground;
  /* physics options */
  double  timestep;
  double  gravity[3];
  double  solref[2];                  /* timeconst, dampratio              */
  double  solimp[5];                  /* dmin, dmax, width, midpoint, power */
  int32_t pgs_iterations;             /* sweeps of the oracle's PGS cross-check (the engine: Newton) */
  double  mpr_tolerance;
  int32_t mpr_iterations;
  /* gripper dimensions used by the env logic (JointSettings::Dim) */
  double  finger_length, finger_width, finger_thickness, finger_E, finger_EI;
  double  segment_length, hook_length, hook_angle_degrees, fingertip_clearance;
  double  yield_stress;
  int32_t fixed_first_segment;
  /* PD gains (JointSettings::ctrl, myfunctions.cpp:273-296) */
  double  kp_gripper[3], kd_gripper[3], kp_base[3], kd_base[3];
  double  time_per_step;              /* stepper chunk: num_steps / pulses_per_s */
  int32_t stepper_num_steps;
  /* gauge (JointSettings::gauge, myfunctions.cpp:264-270) */
  double  gauge_xpos;
  int32_t gauge_order;
  /* tip loading for the gauge calibration (get_segment_matrices / apply_segment_force,
   * myfunctions.cpp:1521-1610, 1660-1727): the last link of each finger and the finger's
   * bending direction at the keyframe (world frame, radially outward) */
  int32_t body_tip[3];
  double  tip_dir[3][3];
  /* gm_model_params.mujoco_actuators */
  int32_t mujoco_actuators;
  /* Newton iterations per constraint solve (0: GM_NEWTON_MAXIT): a test knob that makes
   * capped solves happen (their qacc is no optimum; mj_Euler then integrates qfrc_smooth +
   * J^T efc, not M qacc, see euler_damping) */
  int32_t newton_maxit;
} gm_model;

/* one graspable object (a synthetic object-set entry) */
typedef struct gm_object {
  int32_t type;                       /* GM_GEOM_BOX / _CYLINDER / _SPHERE  */
  double  size[3];                    /* MuJoCo geom size semantics (half sizes) */
  double  mass;
  double  friction;
} gm_object;

/* per-env spawn request: MjClass::spawn_object(index, x, y, zrot) (mjclass.cpp:2352-2420) */
typedef struct gm_spawn {
  int32_t object_index;
  double  x, y, zrot;
} gm_spawn;

/* spawn search request: MjType::SpawnParams (mjclass.h:916-931), defaults as there
 * (gm_default_spawn_params).  The xy grid holds at most GM_SPAWN_MAX_XY points and the
 * rotation grid GM_SPAWN_MAX_ROT (gm_spawn_into_scene rejects larger grids). */
typedef struct gm_spawn_params {
  int32_t index;
  int32_t pad;
  double  x, y, zrot;
  double  xrange, yrange, rotrange;
  double  xmin, xmax, ymin, ymax;
  double  smallest_gap;
  double  xy_increment, rot_increment;
} gm_spawn_params;
#define GM_SPAWN_MAX_XY  1024
#define GM_SPAWN_MAX_ROT 256

/* ------------------------------------------------------------ C ABI */
typedef struct gm_ctx gm_ctx;

/* library / build information */
const char* gm_version(void);
int  gm_device_count(void);
/* sizes of the interface structs (0 settings, 1 model, 2 config, 3 object, 4 spawn,
 * 5 model params, 6 spawn params, 7 calibration, 8 DQN optimiser options) so bindings can verify
 * their layouts */
int64_t gm_struct_size(int which);
/* model summary: nq, nv, nbody, ngeom, npair, n_seg, dof_base, dof_palm, dof_obj,
 * dof_pris[3], dof_rev[3], dof_seg[3], nlock, nM (tree-sparse M nonzeros)  (20 int32) */
void gm_model_info(const gm_model* m, int32_t* out);
/* derived config summary: n_obs, n_actions, sim_steps_per_action, sensor_fcn, state_fcn */
void gm_config_info(const gm_config* c, int32_t* out);

/* Model builder: the MJCF the reference loads with mj_loadXML
 * (mjclass.cpp:377-409) is unavailable (empty `description` submodule), so the
 * gripper is compiled from its numeric parameters instead. */
void gm_default_model_params(gm_model_params* p);
int  gm_build_model(const gm_model_params* p, gm_model* out);

/* MJCF.  The reference compiles its task MJCF with mj_loadXML
 * (mjclass.cpp:377-409), finds everything by the JointSettings / ObjectHandler names
 * (myfunctions.cpp:176-196, 719-787; objecthandler.cpp:22-133) and reads the gripper
 * numerics from <custom><numeric> (read_gripper_dimensions, myfunctions.cpp:836-953).
 * gm_model_to_mjcf writes a model as MJCF with those names (returns the text length;
 * writes it, NUL-terminated, when cap > length); gm_model_from_mjcf compiles the MJCF
 * subset it uses (option, default geom solref/solimp, custom numerics, body / joint
 * slide|hinge|free / inertial / geom plane|sphere|cylinder|box|capsule, contact pairs,
 * equality joint locks, the "initial pose" keyframe) into a gm_model.  A written model
 * reads back identical bit for bit.  err (optional): a message on failure. */
int64_t gm_model_to_mjcf(const gm_model* m, char* buf, int64_t cap);
int  gm_model_from_mjcf(const char* xml, gm_model* out, char* err, int err_cap);

/* Settings defaults (simsettings.h) and derived configuration
 * (MjClass::configure_settings, mjclass.cpp:97-314). */
void gm_default_settings(gm_settings* s);
int  gm_configure(const gm_settings* s, const gm_model* m, gm_config* out);

/* MjClass::set_base_XYZ_limits / set_base_yaw_limit (mjclass.cpp:3847-3859 ->
 * luke::set_base_XYZ_limits / set_base_yaw_limit, myfunctions.cpp:2309-2333): symmetric
 * base operating limits [-x, x], [-y, y], [-z, z] (m) and, when yaw >= 0, [-yaw, yaw]
 * (rad) in a configuration; push it to a context with gm_update_config. */
int  gm_config_set_base_limits(gm_config* cfg, double x, double y, double z, double yaw);

/* Synthetic object sets (the reference's set6/set9 MJCF sets are unavailable). */
int  gm_make_object_set(const char* name, uint64_t seed, gm_object* out, int max_objects);

/* The automatic settings of MjClass::configure_settings (mjclass.cpp:241-308), found by
 * simulation: find_highest_stable_timestep (mjclass.cpp:4745-4854) and
 * calibrate_simulated_sensors (4643-4676, tip load via validate_curve_under_force
 * 4023-4105).  Timesteps keep the reference's float arithmetic. */
typedef struct gm_calibration {
  double  timestep;                   /* s_.mujoco_timestep after the search (and any 0.8x
                                         gauge-run retries, mjclass.cpp:4080)            */
  int32_t sim_steps_per_action;       /* ceil(time_for_action / timestep) (mjclass.cpp:306) */
  int32_t n_tested;                   /* candidate timesteps simulated by the search      */
  double  search_timestep;            /* highest stable timestep found (before the factor) */
  double  yield_load;                 /* calc_yield_point_load (myfunctions.cpp:3587-3595), N */
  double  bend_gauge_normalise;       /* saturation_yield_factor * yield_load (mjclass.cpp:278) */
  float   bending_normalise;          /* gauge reading under that tip load (mjclass.cpp:4666) */
  float   sim_gauge_raw_to_N_factor;  /* mjclass.cpp:281                                   */
  float   wrist_Z_offset;             /* mjclass.cpp:4659: userdata[2] is never written, 0  */
  int32_t gauge_retries;              /* 0.8x timestep retries of the tip-load run          */
} gm_calibration;
/* calibrate_reset's first-call settle as the reference scopes it (myfunctions.cpp:1441-1519:
 * a function-static first_call, so the 400-substep settle runs once per PROCESS and later
 * models with the same joint count reuse its equilibrium even when their timestep or finger
 * stiffness differ).  on = 1: contexts created from now on share one settle (the first one
 * made after the call); 0 (default): every context settles its own model. */
void gm_set_settle_cache(int on);

#define GM_CAL_TIMESTEP 1
#define GM_CAL_GAUGES   2
/* validate_curve_under_force's retry as the reference runs it (mjclass.cpp:4073-4090): on
 * instability the timestep drops to 0.8x, reset() wipes the tip load, and `continue` resumes
 * the step loop -- the remaining steps run unloaded from the reset pose.  Without the flag
 * the whole loaded settle is rerun at the reduced step (the engine's default). */
#define GM_CAL_REFERENCE_RETRY 4
#define GM_CAL_MAX_TRACE 256

/* Batched calibration on `device`: every candidate timestep of the search is simulated
 * for 1 s as its own env in one launch (per-env timestep, mjWARN_BADQACC-style
 * instability flag), and the search replays the reference's coarse/fine sequence over the
 * results, so the answer equals the sequential search.  The gauge run is one env under
 * the saturation tip load for 50 s of simulated time.  `what`: GM_CAL_TIMESTEP |
 * GM_CAL_GAUGES (the gauge run uses model->timestep when the search is off).  trace_dt /
 * trace_unstable (optional, max_trace entries): the search's candidates in order.
 * Sensor and base-position noise are off during calibration. */
int  gm_calibrate(const gm_model* model, const gm_config* cfg, const gm_object* objects, int n_objects,
                  int device, int what, gm_calibration* out, double* trace_dt, uint8_t* trace_unstable,
                  int max_trace);

/* Context lifetime: MjClass() + load() + init() (bind.cpp:46-52, mjclass.cpp:8-95) */
int  gm_create(const gm_model* model, const gm_config* cfg, const gm_object* objects,
               int n_objects, int n_envs, int env_offset, int device, uint64_t seed,
               gm_ctx** out);
void gm_destroy(gm_ctx* ctx);
const char* gm_last_error(const gm_ctx* ctx);
int  gm_n_envs(const gm_ctx* ctx);
int  gm_n_obs(const gm_ctx* ctx);        /* MjClass::get_n_obs     (bind.cpp:157) */
int  gm_n_actions(const gm_ctx* ctx);    /* MjClass::get_n_actions (bind.cpp:156) */
int  gm_update_config(gm_ctx* ctx, const gm_config* cfg);  /* mj.set.* writes */

/* MjClass::reset() (mjclass.cpp:434-486) for envs with mask[e] != 0 (NULL = all),
 * followed by spawn_object(spawn[e]) (mjclass.cpp:2352-2420).  Host arrays. */
int  gm_reset(gm_ctx* ctx, const uint8_t* mask, const gm_spawn* spawn);
/* MjClass::spawn_object(idx, x, y, zrot) alone (mjclass.cpp:2352-2420; bind.cpp:98-105):
 * replaces the live object of masked envs; consumes no RNG draws.  Host arrays. */
int  gm_spawn_object(gm_ctx* ctx, const uint8_t* mask, const gm_spawn* spawn);
/* MjType::SpawnParams defaults (mjclass.h:916-931). */
void gm_default_spawn_params(gm_spawn_params* p);
/* MjClass::spawn_into_scene(SpawnParams) (mjclass.cpp:2475-2654; bind.cpp:100-103) on the
 * device for envs with mask[e] != 0 (NULL = all): the xy and rotation grids are shuffled
 * with std::shuffle semantics on the env's RNG stream, every candidate pose is tested with
 * the Box2d SAT rules (customtypes.h:35-172) against the scene bounds and the initial
 * fingertip boxes (Env::reset, mjclass.h:895-904, from get_finger_hook_locations,
 * myfunctions.cpp:3717-3761), and the object is spawned at the first free pose
 * (spawn_object).  params: n_params == 1 (shared) or n_envs entries.  ok[e] = 1 when
 * spawned, 0 when no pose is free (state unchanged apart from the RNG draws, as in the
 * reference); ok may be NULL.  Host arrays.  The device env holds one live object, so
 * the reference's loop over objects already in the scene is empty (MjEnv._spawn_object
 * spawns one object per reset). */
int  gm_spawn_into_scene(gm_ctx* ctx, const uint8_t* mask, const gm_spawn_params* params, int n_params,
                         uint8_t* ok);
/* Make gm_reset / gm_autoreset place each reset env's object the way MjEnv._spawn_object
 * does (MjEnv.py:1177-1267): spawn_into_scene(spawn[e].object_index) with *params, up to
 * max_tries attempts, falling back to spawn_object(spawn[e]) (MjEnv's "old method").
 * params == NULL restores plain spawn_object(spawn[e]). */
int  gm_set_scene_spawn(gm_ctx* ctx, const gm_spawn_params* params, int max_tries);

/* MjEnv._spawn_object's Python-side draws (MjEnv.py:1177-1267) made per reset on the
 * device: with enable != 0, gm_reset / gm_autoreset called without a spawn table draw each
 * reset env's object index uniformly over the set and its fallback ("old method") pose
 * -- integer-mm x, y in [-position_noise_mm, position_noise_mm], z rotation one of
 * {0, 60, 120} deg plus integer-degree noise in [-rotation_noise_deg, rotation_noise_deg]
 * -- from splitmix64(seed, global env id, episode, draw) (gm_state.h gm_spawn_int), so
 * every episode gets a fresh object, results do not depend on how envs are sharded, and
 * the reference's C++ RNG stream is not consumed.  With gm_set_scene_spawn the drawn index
 * goes to spawn_into_scene first, as MjEnv does. */
int  gm_set_random_spawn(gm_ctx* ctx, int enable, uint64_t seed, int position_noise_mm, int rotation_noise_deg);

/* MjClass::set_motor_target(x, y, z) (bind.cpp:82; mjclass.cpp:1359-1364 ->
 * luke::set_gripper_target_m, myfunctions.cpp:2347-2355 -> Gripper::set_xyz_m, gripper.h:152):
 * the gripper's motor-position target in metres for envs with mask[e] != 0 (NULL = all);
 * the stepper walks toward it over the following action_step()s.  xyz: 3 doubles shared
 * (n_xyz == 1) or 3 per env (n_xyz == n_envs), host array.  in_limits[e] (may be NULL) is
 * the reference's return value: 0 when a motor limit clamped the target.  Used by the
 * reference's force-measurement programs (mysimulate.cpp:2720-2811). */
int  gm_set_motor_target(gm_ctx* ctx, const uint8_t* mask, const double* xyz, int n_xyz, uint8_t* in_limits);
/* MjClass::sim_sensors_SI_ (mjclass.cpp:741-898, read through SensorData::read_finger1_gauge
 * etc., bind.cpp:1149-1151): the latest SI reading of every env, out[e * 5 + k] for k =
 * finger 1..3 bending gauge (N, the raw gauge times sim_gauge_raw_to_N_factor), palm (N),
 * wrist Z (N).  Host array [n_envs x 5]. */
int  gm_get_sensor_si(gm_ctx* ctx, float* out);

/* Synthetic driver for benchmarks and parity tests (not a reference interface): the
 * scripted grasp mix -- per env and episode, phase lengths from splitmix64(seed, global
 * env id, episode); close the fingers, squeeze, press the palm, lift the base, indexed by
 * the env's episode step, plus uniform jitter -- written as continuous action fractions
 * [n_envs x n_actions] to `out` (a device pointer when on_device; feed it to
 * gm_set_action).  Runs on the context's stream after whatever reset came before it. */
int  gm_scripted_actions(gm_ctx* ctx, uint64_t seed, float jitter, float* out, int on_device);
/* Synthetic driver (not a reference interface): uniform random action fractions U[-1, 1)
 * per env and action from a counter-based hash of (seed, global env id, episode, episode
 * step, action index) -- the north star's "synthetic random-action rollouts" -- written like
 * gm_scripted_actions. */
int  gm_random_actions(gm_ctx* ctx, uint64_t seed, float* out, int on_device);
/* Synthetic driver (not a reference interface): the grasp-lift-hold program (mode 3) or the
 * benchmark mix (mode 4: the program in 1 episode of 4 per env -- draw 21 of the episode's
 * counter-based hash -- the scripted grasp mix with `jitter` otherwise) for the current
 * state of every env, written like gm_scripted_actions.  The program is closed-loop and
 * stateless (gm_state.h gm_program_fraction): close, squeeze, lift the base, lower the palm
 * onto the object and hold the palm reading in the stable band -- the reference's success
 * chain (mjclass.cpp:1148-1210, 1295-1322).  GM_E_ARG for another mode. */
int  gm_program_actions(gm_ctx* ctx, uint64_t seed, float jitter, int mode, float* out, int on_device);

/* MjClass::set_continous_action for every action index i in order
 * (mjclass.cpp:1517-1630; called per index by MjEnv._set_action, MjEnv.py:591-594).
 * actions: [n_envs x n_actions] float32.  Host actions are copied into a pinned staging
 * buffer before the call returns (the caller may reuse its array at once); the upload and
 * the action kernel run asynchronously on the context's stream. */
int  gm_set_action(gm_ctx* ctx, const float* actions, int on_device);
/* MjClass::set_discrete_action (mjclass.cpp:1510-1515). actions: [n_envs] int32. */
int  gm_set_discrete_action(gm_ctx* ctx, const int32_t* actions, int on_device);

/* MjClass::action_step() (mjclass.cpp:1483-1508) + get_observation (1700-1959)
 * + is_done (1632-1698) + reward (3000-3049), fused in one device launch,
 * evaluated in the order MjEnv.step uses them (obs, done, reward). */
int  gm_step(gm_ctx* ctx);

int  gm_get_obs(gm_ctx* ctx, float* out, int on_device);                 /* [n_envs x n_obs] */
int  gm_get_reward_done(gm_ctx* ctx, float* reward, uint8_t* done, int on_device);
/* The three at once into host buffers, one stream synchronisation (the facade's
 * get_observation_numpy / is_done / reward of one transition). */
int  gm_get_outputs(gm_ctx* ctx, float* obs, float* reward, uint8_t* done);
/* EventTrack rows: [n_envs x (GM_N_BINARY + GM_N_LINEAR)] int32 `row`, and
 * `abs` counters; MjClass::get_event_state / EventTrack (bind.cpp:525-590). */
int  gm_get_event_rows(gm_ctx* ctx, int32_t* rows, int32_t* abs_counts, float* last_values);
/* raw state readback (testing / checkpoint), fp64 like mjData's qpos / qvel:
 * qpos [n_envs x nq], qvel [n_envs x nv], time [n_envs] (MjClass::get_state-style access
 * the reference's tests use through mjData) */
int  gm_get_state(gm_ctx* ctx, double* qpos, double* qvel, double* time);
int  gm_set_state(gm_ctx* ctx, const double* qpos, const double* qvel);
/* The whole per-env state (everything an MjClass carries between action_step() calls:
 * mjData qpos/qvel/time, target_ stepper state, sensor windows, event tracks, RNG,
 * function-static flags), fp64 where the reference is: gm_env_state_size() bytes per env,
 * [n_envs] records.  Checkpoint / resume, and the hand-off the parity tests use to run
 * the CPU oracle from exactly the device's state.  Host buffers. */
int64_t gm_env_state_size(void);
int  gm_get_env_states(gm_ctx* ctx, void* out);
int  gm_set_env_states(gm_ctx* ctx, const void* in);
/* target (stepper) state: [n_envs x 8] = end x,y,z,th (m/rad) then step x,y,z and base z */
int  gm_get_target(gm_ctx* ctx, double* end_xyzth, int32_t* end_steps, int32_t* next_steps,
                   double* base_xyz);
/* number of envs whose contact list overflowed GM_MAX_CON in the last gm_step */
int  gm_get_overflow(gm_ctx* ctx, int32_t* counts);

/* device pointers for zero-copy (torch.from_blob-style) access */
void* gm_device_obs(gm_ctx* ctx);
void* gm_device_reward(gm_ctx* ctx);
void* gm_device_done(gm_ctx* ctx);
void* gm_device_actions(gm_ctx* ctx);
void* gm_stream(gm_ctx* ctx);
/* route every later launch of ctx to `stream` (a hipStream_t, e.g. torch's current
   stream) so device-pointer I/O is ordered with the caller's work; NULL restores
   the ctx's own stream.  Synchronises the previous stream first. */
int  gm_set_stream(gm_ctx* ctx, void* stream);
/* MjEnv's episode-boundary handling done on the device (MjEnv.py:616-637 then
 * MjEnv.reset, MjEnv.py:2222-2263): every env with done != 0 from the last gm_step,
 * or num_action_steps >= max_episode_steps (<= 0 disables truncation), writes its
 * cumulative reward to returns[e] (NaN for envs that continue; returns may be NULL),
 * is flagged in gm_device_reset_mask, and is reset + respawned from spawn[e].
 * spawn: host array unless spawn_on_device; NULL spawns object 0 at the origin. */
int  gm_autoreset(gm_ctx* ctx, int max_episode_steps, const gm_spawn* spawn, int spawn_on_device,
                  float* returns);
void* gm_device_reset_mask(gm_ctx* ctx);   /* uint8 [n_envs], written by gm_autoreset */
/* The episode-end record north_star's RCCL all-gather carries: per env, the
 * episode return (MjEnv's cumulative reward, MjEnv.py:616-637), its length in env-steps
 * (MjClass::env_.num_action_steps) and success -- the reference's successful_grasp metric
 * (mjclass.cpp:1295-1322: a +1-reward, done-setting binary event triggered this step).  Envs
 * whose episode continues hold {NaN, 0, 0}.  12 bytes, so a [n_envs] array is a plain
 * [n_envs x 3] 4-byte tensor for the collective. */
typedef struct gm_episode_end {
  float   ret;
  int32_t length;
  uint8_t success;
  uint8_t pad[3];
} gm_episode_end;
/* gm_autoreset that also writes the episode-end record of every env (device array
 * [n_envs], may be NULL) -- returns may be NULL too. */
int  gm_autoreset_episodes(gm_ctx* ctx, int max_episode_steps, const gm_spawn* spawn, int spawn_on_device,
                           float* returns, gm_episode_end* episodes);

/* A fused batched rollout (the env-step hot path with its synthetic driver on the device):
 * n_steps repetitions, for every env, of exactly the per-step API's sequence
 *   gm_scripted_actions (action_mode 0, seed, jitter), gm_random_actions (1, seed) or
 *   gm_program_actions (3: the grasp program, 4: the benchmark's program / scripted mix)
 *   -> gm_set_action -> gm_step -> gm_autoreset_episodes(max_episode_steps, spawn = NULL,
 *      records + k * n_envs)
 * -- the same code on the same state, so the results are bit for bit those of the n_steps
 * per-step calls -- but as ONE persistent launch: an env that finishes env-step k starts k + 1
 * at once on its wave (actions, the termination lift's extra substeps, the episode-end record
 * and MjEnv.reset's reset + spawn included) while the work queue balances envs at substep
 * granularity, so the launch's tail is paid once per n_steps env-steps instead of every step.
 * records: device array [n_steps x n_envs] (or NULL); obs / reward / done buffers hold the last
 * env-step's (the reset observation for envs reset at its end), as after the per-step calls. */
typedef struct gm_rollout_params {
  int32_t  action_mode;        /* 0: scripted grasp mix, 1: uniform random, 3: grasp program,
                                  4: program in 1 episode of 4, scripted mix otherwise
                                  (2 and 5 are the launch's internal codes for gm_policy_rollout
                                  and gm_ac_rollout; gm_rollout rejects them) */
  int32_t  max_episode_steps;  /* MjEnv truncation; <= 0 disables it */
  uint64_t seed;
  float    jitter;             /* scripted mode only */
  int32_t  pad;
} gm_rollout_params;
int  gm_rollout(gm_ctx* ctx, int n_steps, const gm_rollout_params* params, gm_episode_end* records);

/* Timing of the last env-step kernel launch (HIP events on the context's stream): a gm_step
 * (one env-step per env) or a gm_rollout / gm_policy_rollout launch of n_steps env-steps per
 * env -- gm_dispatch_info out[3] says which; divide by it for a per-env-step figure.
 * gm_chunk_stats and gm_chunk_timeline likewise describe that last launch. */
int  gm_last_step_ms(gm_ctx* ctx, float* ms);
/* The last gm_step's work queue (chunked dispatch): out[0] envs started,
 * out[1] envs finished, out[2] yields (an env handed back to its XCD's queue because an
 * unstarted env had more work left), out[3] resumptions; out[4] substeps between
 * preemption tests (0: the one-shot kernel ran), out[5] resident workgroups, out[6] the
 * resumptions by a wave of another XCD than the yielding one's.  times (may
 * be NULL; 100 MHz constant-clock ticks): [0] first pick, [1] first pick that found no
 * unstarted env, [2] last env finished, [3] sum of wave-busy time, [4] sum of wave polling.
 * Synchronises the context's stream. */
int  gm_chunk_stats(gm_ctx* ctx, uint32_t* out7, uint64_t* times5);
/* The last chunked launch's claim waits: out[0] claims of a yielded env's ring slot that found
 * the slot still empty (its producer between the tail increment and the entry store), out[1]
 * the polls those claims made.  A claimed slot always has a producer in flight
 * (claim_bucket's invariant), so the polls per waiting claim stay small; a claim parked on a
 * slot only a future yield would fill shows as a run of polls.  Synchronises the stream. */
int  gm_chunk_claim_waits(gm_ctx* ctx, uint32_t* out2);
/* The last chunked launch's jobs, per env (arrays of n_envs, either may be NULL): clk[e] the
 * shader clocks / 64 (s_memtime) env e's job ran for, summed over its chunks; yields[e] how
 * often the job was handed back to the queue.  Set when a job finishes (an env the launch
 * did not reach keeps the previous value).  Synchronises the context's stream.  Diagnostics:
 * a job's work against its life (gm_chunk_timeline). */
int  gm_chunk_job_stats(gm_ctx* ctx, uint32_t* clk, int32_t* yields);
/* How gm_step / gm_rollout dispatch this context (fixed at gm_create): out[0] substeps
 * between preemption tests (0: the one-shot kernel), out[1] workgroups of the chunked
 * grid, out[2] waves per env (1; 2 = DUO workgroups, whose second wave runs the collider
 * concurrently -- chosen when every env's two waves fit resident, GM_DUO=0/1 forces it),
 * out[3] env-steps per env of the last launch (1 after gm_step, n_steps after a rollout:
 * the unit of gm_last_step_ms / gm_chunk_stats / gm_chunk_timeline). */
int  gm_dispatch_info(const gm_ctx* ctx, int32_t* out4);
/* The last chunked launch's per-workgroup end of work: when workgroup w finished the last
 * env (or env chunk) it ran, before it polled out the rest of the launch (100 MHz constant
 * clock, the clock of gm_chunk_stats' times, in the low 60 bits; the workgroup's XCD in
 * the top 4): out[w] for w < G = out[1] of gm_dispatch_info; then, per env e, when it was first
 * picked and when its job finished: out[G + 2 e], out[G + 2 e + 1] (up to max_out words).  Returns the count written (>= 0) or a negative error.  Synchronises
 * the context's stream.  Diagnostics: the shape of the launch's tail. */
int  gm_chunk_timeline(gm_ctx* ctx, uint64_t* out, int max_out);

/* ---- single-substep stage hooks for parity testing (GPU vs oracle) ---- */
/* Runs exactly one MjClass::step (mj_step1 + control + mj_step2 + mj_rnePostConstraint
 * equivalent, then update_all and monitor_sensors; mjclass.cpp:504-530) on every env,
 * from the current state, and copies out fp64 diagnostics (any pointer may be NULL):
 * ncon[n_envs], contact [n_envs x GM_MAX_CON x 16] (dist, pos3, frame9, g1, g2, mu),
 * efc_force [n_envs x GM_MAX_EFC], qacc [n_envs x GM_MAX_DOF], nefc [n_envs], and
 * obj_wrench [n_envs x 6]: the live object's cfrc_ext as
 * ObjectHandler::get_object_net_force_faster returns it (objecthandler.cpp:543-565),
 * [force; torque about its centre of mass]. */
int  gm_debug_substep(gm_ctx* ctx, int32_t* ncon, double* contact, double* efc_force,
                      double* qacc, int32_t* nefc, double* obj_wrench);
/* diagnostic: one gm_step with per-phase shader-clock cycle counters, lane-0 view,
   summed over substeps: out[n_envs][32]; columns 0-27 are clocks (names in gmx.env
   BatchedGripperEnv.PHASES: kinematics, crb_rne, mass+forces, collision, newton_solve,
   integrate, update_all, monitor_sensors, the Newton sub-phases, the env-step epilogue),
   28 = constraint rows summed, 29 = substeps that ran MPR, 30 = Newton iterations,
   31 = line-search evaluations */
int  gm_step_profiled(gm_ctx* ctx, uint64_t* phase_cycles);

/* ---- on-device DQN policy ----
 * VariableNetwork.forward (rl/networks.py:7-41: Linear+ReLU hidden layers, final Linear,
 * Softmax(dim=1)) on every env's current observation, then Agent_DQN.select_action
 * (rl/agents/DQN.py:184-209): argmax of the network output, or with probability eps a
 * uniform random action.  The chosen discrete actions are applied to the envs on the
 * device (MjClass::set_discrete_action), so a rollout needs no host round trip.
 * sizes: n_sizes layer widths [n_obs, hidden..., n_actions] (<= 8 layers, widths <= 256);
 * params: torch state_dict order, f32 -- W0 [sizes[1] x sizes[0]] row-major, b0
 * [sizes[1]], W1, b1, ...  (host pointer). */
typedef struct gm_policy gm_policy;
int  gm_policy_create(gm_ctx* ctx, const int32_t* sizes, int n_sizes, const float* params,
                      gm_policy** out);
void gm_policy_destroy(gm_policy* p);
/* Host-side repack of params into the device layout (MFMA B-fragment order, zero
 * padded); returns the packed float count, writes `out` when non-NULL.  Exposed so the
 * layout is testable without a GPU. */
int64_t gm_policy_pack(const int32_t* sizes, int n_sizes, const float* params, float* out);
/* select (eps-greedy, counter-based per-env draws from (seed, global env id, decision))
 * and apply actions for every env; eps = eps_threshold of select_action */
int  gm_policy_act(gm_policy* p, float eps, uint64_t seed, uint64_t decision);
/* last selected actions [n_envs] int32 and softmax outputs [n_envs x n_actions] f32
 * (either may be NULL); host copies */
int  gm_policy_read(gm_policy* p, int32_t* actions, float* q);
/* A fused on-device DQN rollout: n_steps repetitions, for every env, of
 *   gm_policy_act(p, eps[k], seed, decision0 + k) -> gm_step
 *   -> gm_autoreset_episodes(max_episode_steps, spawn = NULL, records + k * n_envs)
 * as ONE persistent launch of gm_rollout's kind: each env's own wave runs select_action on
 * its observation (the batched kernel's MFMA tiles with the env in row 0 -- rows are
 * independent, so the action is bit for bit the batched kernel's) before each env-step.
 * Results (state, observations, records) equal the per-step sequence's bit for bit.
 * eps: host array [n_steps] (copied before the call returns); records: device array
 * [n_steps x n_envs] or NULL.  gm_policy_read's buffers are not written by the fused
 * launch (they are under GM_CHUNK_SUBSTEPS=0, which runs the per-step sequence). */
int  gm_policy_rollout(gm_policy* p, int n_steps, const float* eps, uint64_t seed, uint64_t decision0,
                       int max_episode_steps, gm_episode_end* records);
/* New weights after a learner update (Agent_DQN.optimise_model's optimiser step, or the soft
 * target update of update_step, rl/agents/DQN.py:352-360): same layout as gm_policy_create's
 * params; copied before the call returns.  A target network is a second gm_policy on the same
 * context. */
int  gm_policy_set_params(gm_policy* p, const float* params);

/* ---- DQN replay memory, its draw and the TD target ----
 * ReplayMemory (rl/agents/DQN.py:11-62): a bounded deque of Transition(state, action, next_state,
 * reward, terminal), filled by Agent_DQN.update_step (:329-348) once per env-step
 * (rl/Trainer.py:659-684, which always passes the real post-step observation as next_state).
 * The memory is the caller's device arrays, a ring of `capacity` rows.  The ring position is the
 * caller's too: every call takes row0, the number of transitions pushed before it, and env e at
 * env-step k of the call writes row (row0 + k * n_envs + e) % capacity -- the deque with every env
 * pushed in env order each env-step; no atomics, no dependence on dispatch.  A call that would
 * write a row twice (n_steps * n_envs > capacity) fails with GM_E_ARG; capacity need not be a
 * multiple of n_envs. */
typedef struct gm_replay {
  int64_t  capacity;    /* rows */
  float*   state;       /* [capacity][n_obs]  observation the action was chosen from */
  int32_t* action;      /* [capacity]         the discrete action taken */
  float*   next_state;  /* [capacity][n_obs]  observation after the env-step, never the reset one */
  float*   reward;      /* [capacity] */
  uint8_t* end;         /* [capacity]  0 episode continues, 1 terminal (done), 2 truncated only */
} gm_replay;
/* a sampled batch: the caller's contiguous device arrays of `batch` rows */
typedef struct gm_replay_batch {
  float*   state;       /* [batch][n_obs] */
  int32_t* action;      /* [batch] */
  float*   next_state;  /* [batch][n_obs] */
  float*   reward;      /* [batch] */
  uint8_t* end;         /* [batch] */
  int32_t* index;       /* [batch] the ring rows gathered */
} gm_replay_batch;
/* ReplayMemory.push in two halves around the env-step.  After gm_policy_act: state (the
 * observation the action was chosen from) and action of every env. */
int  gm_policy_push_begin(gm_policy* p, const gm_replay* replay, int64_t row0);
/* After gm_step and BEFORE the auto-reset: next_state (the post-step observation), reward and
 * end (gm_ac_record's rule: 1 done, else 2 when max_episode_steps > 0 and the episode reached
 * it, else 0), into the rows gm_policy_push_begin(row0) wrote. */
int  gm_policy_push_end(gm_policy* p, const gm_replay* replay, int64_t row0, int max_episode_steps);
/* The fused form: gm_policy_rollout that also records.  For k = 0 .. n_steps - 1
 *   gm_policy_act(eps[k], seed, decision0 + k) -> gm_policy_push_begin(row0 + k * n_envs)
 *   -> gm_step -> gm_policy_push_end(row0 + k * n_envs, max_episode_steps)
 *   -> gm_autoreset_episodes(max_episode_steps, spawn = NULL, records + k * n_envs)
 * as ONE persistent launch; every array of the memory equals the per-step sequence's bit for
 * bit, and state, observations and records equal gm_policy_rollout's with the same arguments.
 * Under GM_CHUNK_SUBSTEPS=0 it runs that sequence.  The caller advances its count of pushed
 * transitions by n_steps * n_envs. */
int  gm_policy_rollout_replay(gm_policy* p, int n_steps, const float* eps, uint64_t seed, uint64_t decision0,
                              int max_episode_steps, gm_episode_end* records, const gm_replay* replay,
                              int64_t row0);
/* ReplayMemory.batch (DQN.py:31-46: random.Random.sample, without replacement) as a counter-based draw:
 * out[i], i < batch, is the image of i under a keyed bijection of [0, size), size = min(pushed,
 * capacity) -- a balanced Feistel network of 4 rounds over the smallest even bit count b with
 * 2^b >= size, round function splitmix64's finaliser of (key + round constant + R) masked to
 * b / 2 bits, key from (seed, draw), cycle-walked until the value is < size.  The rows are
 * distinct; the stream is not the agent's random.Random.  Host only, no GPU needed;
 * batch > size is GM_E_ARG (the reference skips optimisation then, DQN.py:258). */
int  gm_replay_indices(int64_t size, int batch, uint64_t seed, uint64_t draw, int32_t* out);
/* The same indices computed on the device and the rows gathered into out's arrays: one kernel. */
int  gm_replay_sample(gm_ctx* ctx, const gm_replay* replay, int64_t size, int batch, uint64_t seed,
                      uint64_t draw, const gm_replay_batch* out);
/* The TD target of the first n rows of a batch (Agent_DQN.optimise_model, DQN.py:294-315):
 * y = reward + gamma * v, v the maximum of target's softmax outputs on next_state or, with
 * online != NULL (use_double_dqn), target's output at online's first argmax.  mask_terminal = 0
 * is the reference as written (every row bootstraps: its non_final_mask is all true);
 * mask_terminal = 1 sets v = 0 where end == 1 and keeps the bootstrap where end == 2.
 * Reads batch->next_state, reward and end; y, next_value (v; may be NULL): device [n]. */
int  gm_policy_td_target(gm_policy* target, gm_policy* online, const gm_replay_batch* batch, int n, float gamma,
                         int mask_terminal, float* y, float* next_value);

/* ---- DQN learner: backward, Adam / AdamW step and the soft target update ----
 * Agent_DQN.optimise_model from the loss on (rl/agents/DQN.py:317-327: criterion, backward,
 * clip_grad_value_, optimiser.step) and update_step's soft target update (:352-360), on the packed
 * weights where the rollout reads them: gradients and moments live in gm_policy_pack's layout, the
 * step updates the online policy in place, nothing is repacked and no weight crosses the bus.
 * f32; no float atomics: the same call on the same inputs gives the same bits.  RMSprop (:130-132)
 * and update_episode's hard-copy schedule are not here; a hard copy is gm_policy_soft_update with
 * tau = 1. */
#define GM_OPT_ADAM        0    /* torch.optim.Adam  (DQN.py:133-137) */
#define GM_OPT_ADAMW       1    /* torch.optim.AdamW (DQN.py:138-143) */
#define GM_LOSS_SMOOTH_L1  0    /* nn.SmoothL1Loss(), beta 1 = nn.HuberLoss(), delta 1 (DQN.py:146-151) */
#define GM_LOSS_MSE        1    /* nn.MSELoss() */
#define GM_LEARNER_MAX_BATCH 256
typedef struct gm_dqn_opt {     /* Agent_DQN.Parameters (DQN.py:68-92) as init() hands them to torch (:130-151);
                                   doubles, as torch keeps its hyperparameters */
  int32_t optimiser;            /* GM_OPT_* */
  int32_t amsgrad;
  int32_t loss;                 /* GM_LOSS_* */
  int32_t pad;
  double  lr, beta1, beta2, eps, weight_decay;
  double  grad_clamp;           /* clip_grad_value_'s bound (DQN.py:325-326); <= 0: none */
} gm_dqn_opt;
/* Parameters' defaults as torch resolves them: AdamW, lr 1e-4, betas (0.9, 0.999), eps 1e-8,
 * weight_decay 0.01 (torch's AdamW default), amsgrad on, smooth-L1, clamp 100 */
void gm_dqn_opt_default(gm_dqn_opt* out);
/* A learner for `online`, on its context: owns the per-tile partial gradients, the summed gradient,
 * exp_avg / exp_avg_sq / max_exp_avg_sq (zero), the step count (0) and the scratch, sized for
 * batches of up to GM_LEARNER_MAX_BATCH rows.  Destroy it before `online`. */
typedef struct gm_learner gm_learner;
int  gm_learner_create(gm_policy* online, const gm_dqn_opt* opt, gm_learner** out);
void gm_learner_destroy(gm_learner* l);
/* loss.backward() (DQN.py:292, 319-323) for the first n rows of a batch: q_a = softmax(net(state))
 * [action], loss = mean criterion(q_a, y); leaves the raw, unclamped gradient (packed) and the mean
 * loss on the device.  Reads batch->state and batch->action; y: device [n].  n > GM_LEARNER_MAX_BATCH
 * is GM_E_ARG. */
int  gm_learner_grad(gm_learner* l, const gm_replay_batch* batch, const float* y, int n);
/* clip_grad_value_ and optimiser.step() (DQN.py:325-327) on the held gradient, in place on the
 * online policy's device weights; the step count goes up by one. */
int  gm_learner_step(gm_learner* l);
/* The held gradient in gm_policy_create's flat order and the mean loss (host pointers; either may
 * be NULL). */
int  gm_learner_read(gm_learner* l, float* grad_flat, float* loss);
/* optimiser.state_dict()'s tensors in flat order (DQN.py saves optimiser_state_dict with the
 * agent): step, exp_avg, exp_avg_sq, max_exp_avg_sq.  Host pointers; any may be NULL. */
int  gm_learner_get_state(gm_learner* l, int64_t* step, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq);
int  gm_learner_set_state(gm_learner* l, const int64_t* step, const float* exp_avg, const float* exp_avg_sq,
                          const float* max_exp_avg_sq);
/* The inverse of gm_policy_set_params: the device weights in flat order (host pointer). */
int  gm_policy_get_params(gm_policy* p, float* flat);
/* The device weights as stored, gm_policy_pack's layout and count (host pointer): the padding
 * entries included, which must stay exactly 0 under every update. */
int  gm_policy_get_packed(gm_policy* p, float* packed);
/* target <- tau online + (1 - tau) target (DQN.py:352-360) on the device; the two policies need
 * the same layer sizes and the same context.  tau = 1 copies online bit for bit. */
int  gm_policy_soft_update(gm_policy* target, gm_policy* online, float tau);
/* n_updates learning steps enqueued with no host synchronisation between them: for u = 0 ..
 * n_updates - 1
 *   gm_replay_sample(size, batch, seed, draw0 + u) into the learner's own batch arrays
 *   -> gm_policy_td_target(target, double_dqn ? online : NULL, gamma, mask_terminal)
 *   -> gm_learner_grad -> gm_learner_step -> gm_policy_soft_update(target, online, tau)
 * the same kernels in the same order as the calls, so every result equals theirs bit for bit.
 * target = NULL: the online net is its own target (then tau must be <= 0); tau <= 0 skips the
 * soft update.  losses: device [n_updates] (the mean loss of every update) or NULL. */
int  gm_learner_train(gm_learner* l, gm_policy* target, const gm_replay* replay, int64_t size, int batch,
                      uint64_t seed, uint64_t draw0, int n_updates, float gamma, int double_dqn,
                      int mask_terminal, float tau, float* losses);

/* ---- on-device PPO actor-critic, trajectory buffer and GAE ----
 * MLPActorCriticPG.step (rl/agents/PolicyGradient.py:522-528) and Agent_PPO.select_action
 * (:1348-1386) on every env's current observation:
 *   mu = mu_net(obs) (MLPGaussianActor, :449-471: Linear+Tanh hidden layers, identity output),
 *   std = exp(log_std), a = mu + std z with z ~ N(0, 1),
 *   logp = sum_i ( -(a_i - mu_i)^2 / (2 std_i^2) - log_std_i - 0.5 log(2 pi) )  (Normal.log_prob
 *   summed over the action axis), v = v_net(obs) (MLPCritic, :473-487),
 * then, with noise > 0, uniform noise in [-noise, noise) per action added to a after logp is
 * taken (select_action's exploration noise).  The actions go to the envs on the device through
 * the continuous-action path, which clips to [-1, 1] (MjEnv._set_action, rl/env/MjEnv.py:591-594:
 * set_action_one once per action index, in order); the buffer keeps the unclipped ones.
 * f32, the DQN network's MFMA, packing and limits (<= 8 layers, widths <= 256).  Draws are
 * counter-based per (seed, global env id, decision, action index) -- csrc/gm_ac_net.h has the
 * construction, gmx/ppo.py normal_draws / noise_draws its host mirror -- so results do not
 * depend on sharding.
 *
 * The trajectory buffer is the caller's device memory (PPOBuffer, PolicyGradient.py:301-409),
 * time-major so that all envs of one env-step are contiguous. */
typedef struct gm_ac_traj {
  int32_t capacity;   /* env-steps K the arrays hold */
  int32_t pad;
  float*   obs;       /* [K][n_envs][n_obs]   observation the action was chosen from */
  float*   act;       /* [K][n_envs][n_actions] action sent to the env (noisy, unclipped);
                         categorical handle: [K][n_envs][1], the chosen index as a float */
  float*   logp;      /* [K][n_envs] */
  float*   val;       /* [K][n_envs]  V(obs[k]) */
  float*   rew;       /* [K][n_envs]  reward of env-step k */
  uint8_t* end;       /* [K][n_envs]  0 episode continues, 1 terminal (done), 2 truncated only */
  float*   boot;      /* [K][n_envs]  V(observation after env-step k) where end == 2, else 0 */
  float*   last_val;  /* [n_envs]     V(observation after the last recorded env-step) */
  float*   mu;        /* [K][n_envs][n_actions], may be NULL (diagnostics / tests); categorical: the logits */
} gm_ac_traj;
typedef struct gm_ac gm_ac;
/* actor_sizes: [n_obs, hidden..., n_actions]; critic_sizes: [n_obs, hidden..., 1]; params (host,
 * f32): the actor's W0 [sizes[1] x sizes[0]] row-major, b0, W1, b1, ..., then the critic's in
 * the same order, then log_std [n_actions].  Needs continous_actions != 0 (the mirror of
 * gm_policy_create's check); GM_E_ARG with a gm_last_error message for a network that does
 * not map n_obs to n_actions / to 1 or has unsupported sizes. */
int  gm_ac_create(gm_ctx* ctx, const int32_t* actor_sizes, int n_actor, const int32_t* critic_sizes,
                  int n_critic, const float* params, gm_ac** out);
void gm_ac_destroy(gm_ac* p);
/* New weights after a learner update (Agent_PPO.update_step's result): same layout as
 * gm_ac_create's params; copied before the call returns. */
int  gm_ac_set_params(gm_ac* p, const float* params);
/* Host-side repack into the device layout: [actor | critic] each in gm_policy_pack's layout,
 * then log_std.  Returns the packed float count (negative for unsupported sizes), writes `out`
 * when non-NULL.  off2 (may be NULL): the critic's and log_std's float offsets. */
int64_t gm_ac_pack(const int32_t* actor_sizes, int n_actor, const int32_t* critic_sizes, int n_critic,
                   const float* params, float* out, int64_t* off2);
/* select_action for every env from its current observation: fills obs[k], act[k], logp[k],
 * val[k] (and mu[k]) and applies the actions.  sample = 0: a = mu (evaluation; logp is mu's). */
int  gm_ac_act(gm_ac* p, const gm_ac_traj* traj, int k, int sample, float noise, uint64_t seed,
               uint64_t decision);
/* After gm_step and BEFORE the auto-reset: rew[k], end[k] (1 done, else 2 when
 * max_episode_steps > 0 and the episode reached it, else 0) and boot[k] -- the critic on the
 * post-step observation where end == 2 (PPOBuffer.finish_trajectory's last_val of a cut
 * trajectory, Agent_PPO's truncation bootstrap), 0 elsewhere. */
int  gm_ac_record(gm_ac* p, const gm_ac_traj* traj, int k, int max_episode_steps);
/* last_val from the current observations, after env-step k_last's auto-reset. */
int  gm_ac_finish(gm_ac* p, const gm_ac_traj* traj, int k_last);
/* The fused form: for k = 0 .. n_steps - 1
 *   gm_ac_act(k, decision0 + k) -> gm_step -> gm_ac_record(k, max_episode_steps)
 *   -> gm_autoreset_episodes(max_episode_steps, spawn = NULL, records + k * n_envs)
 * then gm_ac_finish(n_steps - 1), as ONE persistent launch of gm_rollout's kind: each env's own
 * wave runs actor and critic (the batched kernels' MFMA tiles with the env in row 0) between
 * its env-steps.  Every result -- state, observations, records and the whole buffer -- equals
 * the per-step sequence's bit for bit.  Under GM_CHUNK_SUBSTEPS=0 it runs that sequence.
 * records: device [n_steps x n_envs] or NULL. */
int  gm_ac_rollout(gm_ac* p, const gm_ac_traj* traj, int n_steps, int sample, float noise, uint64_t seed,
                   uint64_t decision0, int max_episode_steps, gm_episode_end* records);
/* GAE-lambda advantages and rewards-to-go (PPOBuffer.finish_trajectory, PolicyGradient.py:355-380)
 * per env and trajectory segment over the first n_steps rows of traj (reads rew, val, end,
 * boot, last_val only); adv, ret: device [n_steps][n_envs]. */
int  gm_ac_gae(gm_ctx* ctx, const gm_ac_traj* traj, int n_steps, float gamma, float lam, float* adv,
               float* ret);
/* PPOBuffer.get's advantage normalisation (PolicyGradient.py:384-407) in place on a device array:
 * adv <- (adv - mean) / std, std the unbiased standard deviation as torch.std_mean gives it.  The
 * sums are formed in double in a fixed order: the same input gives the same bytes.  n < 2 is
 * GM_E_ARG (the standard deviation of one value is undefined). */
int  gm_ac_adv_normalise(gm_ctx* ctx, float* adv, int64_t n);
/* The inverse of gm_ac_set_params: the device weights in gm_ac_create's flat order (host pointer). */
int  gm_ac_get_params(gm_ac* p, float* flat);
/* The device weights as stored, gm_ac_pack's layout and count (host pointer): the padding entries
 * included, which must stay exactly 0 under every update. */
int  gm_ac_get_packed(gm_ac* p, float* packed);

/* ---- the categorical actor: PPO on discrete actions ----
 * MLPActorCriticPG(continous_actions=False) builds an MLPCategoricalActor (PolicyGradient.py:429-447,
 * :504-509): the same MLP [n_obs, hidden..., n_actions] with its outputs read as logits,
 *   pi = Categorical(logits = logits_net(obs)),  a ~ pi,  logp = pi.log_prob(a) = logits_a - logsumexp
 * and no log_std.  params: the actor's W0, b0, ..., then the critic's; the blob is [actor | critic].
 * Needs continous_actions == 0; GM_E_ARG with a gm_last_error message otherwise, and for an actor
 * that does not map n_obs to gm_n_actions or a critic that does not map n_obs to 1.
 * The handle is a gm_ac: every gm_ac_* and gm_ppo_learner_* call takes it.  With it
 *   gm_ac_traj.act is [K][n_envs][1], the chosen index as a float (PPOBuffer with action_dim 1);
 *   gm_ac_traj.mu, when non-NULL, holds the logits [K][n_envs][n_actions];
 *   gm_ppo_batch.act is [n][1];
 *   noise != 0 is GM_E_ARG (the reference's select_action adds float noise in place to a Long
 *   tensor, which raises: the categorical actor runs with use_random_action_noise = False only);
 *   gm_ac_act applies the index through the discrete-action path, as gm_policy_act does, the
 *   termination action's extra substeps included;  sample = 0 takes the argmax (lowest index on a tie);
 *   the learner's ent is the mean row entropy, its gradient goes through the logits, and the
 *   optimiser state calls carry no log_std entries.
 * One uniform per (seed, global env id, decision) picks the action by the inverse CDF
 * (csrc/gm_ac_net.h ga_sample_cat; gmx/ppo.py categorical_uniforms mirrors the draw). */
int  gm_ac_create_categorical(gm_ctx* ctx, const int32_t* actor_sizes, int n_actor, const int32_t* critic_sizes,
                              int n_critic, const float* params, gm_ac** out);
/* gm_ac_pack without log_std: off2[1] is then the packed count itself. */
int64_t gm_ac_pack_categorical(const int32_t* actor_sizes, int n_actor, const int32_t* critic_sizes,
                               int n_critic, const float* params, float* out, int64_t* off2);

/* ---- PPO learner: clipped-surrogate backward, two Adams, KL stop ----
 * Agent_PPO.optimise_model (rl/agents/PolicyGradient.py:1440-1522) on the packed weights where the
 * rollout reads them: gradients and moments live in gm_ac_pack's layout, the steps update the
 * actor-critic in place, nothing is repacked and no weight crosses the bus.  f32; no float atomics:
 * the same call on the same inputs with the same n_groups gives the same bits.  Full-batch like the
 * reference; RMSprop is not here. */
typedef struct gm_ppo_opt {     /* Agent_PPO.Parameters' learner options (PolicyGradient.py:1196-1220);
                                   doubles, as torch keeps its hyperparameters */
  double  learning_rate_pi, learning_rate_vf, gamma, lam, clip_ratio;
  int32_t train_pi_iters, train_vf_iters;
  double  target_kl, max_kl_ratio;
  int32_t optimiser;            /* GM_OPT_ADAM: Adam(lr, betas); GM_OPT_ADAMW: AdamW(lr, betas, amsgrad=True),
                                   weight_decay 0.01 (torch's default), as Agent_PPO.init passes them */
  int32_t use_kl_penalty;
  double  kl_penalty_coefficient;
  int32_t use_entropy_regularisation;
  int32_t pad;
  double  entropy_coefficient, adam_beta1, adam_beta2;
  double  grad_clamp_value;     /* clip_grad_value_'s bound; <= 0: none (Parameters' None) */
} gm_ppo_opt;
/* Parameters' defaults: lr 3e-4 / 1e-3, gamma 0.99, lam 0.97, clip 0.2, 80 + 80 iterations,
 * target_kl 0.01, max_kl_ratio 1.5, Adam, no KL penalty (0.2), no entropy term (1e-4), betas
 * (0.9, 0.999), no clamp */
void gm_ppo_opt_default(gm_ppo_opt* out);
/* n rows of a batch, device arrays: the first k rows of a trajectory buffer are already in this
 * shape ([k * n_envs] rows). */
typedef struct gm_ppo_batch {
  int64_t n;
  const float* obs;             /* [n][n_obs] */
  const float* act;             /* [n][n_actions]; categorical handle: [n][1], the index as a float */
  const float* logp;            /* [n]  log-probabilities under the policy that collected the rows */
  const float* adv;             /* [n]  (normalised) advantages */
  const float* ret;             /* [n]  rewards-to-go */
} gm_ppo_batch;
typedef struct gm_ppo_info {    /* what one gm_ppo_learner_update did */
  int32_t pi_iters_done;        /* policy iterations that stepped (the KL stop ends them early) */
  int32_t pad;
  float   first[5], last[5];    /* loss_pi, loss_v, kl, ent, cf of the first and of the last iteration
                                   evaluated (policy: the one that stopped, when one did) */
} gm_ppo_info;
/* A learner for `ac`, on its context, with n_groups workgroups per gradient launch (0: the default;
 * its buffers depend on n_groups and the net, never on the batch): owns one partial gradient per
 * workgroup, the summed gradient, both optimisers' exp_avg / exp_avg_sq / max_exp_avg_sq (zero)
 * and step counts (0).  GM_E_ARG with a gm_last_error text for an optimiser other than
 * GM_OPT_ADAM / GM_OPT_ADAMW (RMSprop is not on the device).  Destroy it before `ac`. */
typedef struct gm_ppo_learner gm_ppo_learner;
int  gm_ppo_learner_create(gm_ac* ac, const gm_ppo_opt* opt, int n_groups, gm_ppo_learner** out);
void gm_ppo_learner_destroy(gm_ppo_learner* l);
/* compute_loss_pi's backward (reads obs, act, logp, adv) and compute_loss_v's (reads obs, ret) for
 * the batch: leave the raw gradient of the policy's parameters (actor net, log_std) / the critic's
 * and loss_pi, kl, ent, cf / loss_v on the device.  n < 1 or a missing array is GM_E_ARG. */
int  gm_ppo_learner_grad_pi(gm_ppo_learner* l, const gm_ppo_batch* batch);
int  gm_ppo_learner_grad_vf(gm_ppo_learner* l, const gm_ppo_batch* batch);
/* clip_grad_value_ and pi_optimiser.step() / vf_optimiser.step() on the held gradient, in place on
 * the device weights; that optimiser's step count goes up by one. */
int  gm_ppo_learner_step_pi(gm_ppo_learner* l);
int  gm_ppo_learner_step_vf(gm_ppo_learner* l);
/* The held gradient in gm_ac_create's flat order and loss_pi, loss_v, kl, ent, cf (scalars[5]).
 * Host pointers; either may be NULL. */
int  gm_ppo_learner_read(gm_ppo_learner* l, float* grad_flat, float* scalars);
/* Both optimisers' state in flat order, the policy's entries (actor, log_std) from pi_optimiser
 * and the critic's from vf_optimiser: steps[2] = {pi, vf}.  Host pointers; any may be NULL. */
int  gm_ppo_learner_get_state(gm_ppo_learner* l, int64_t* steps, float* exp_avg, float* exp_avg_sq,
                              float* max_exp_avg_sq);
int  gm_ppo_learner_set_state(gm_ppo_learner* l, const int64_t* steps, const float* exp_avg,
                              const float* exp_avg_sq, const float* max_exp_avg_sq);
/* The whole optimise_model on the first n_steps rows of traj, enqueued with one host read at the end:
 *   gm_ac_gae(gamma, lam) -> gm_ac_adv_normalise
 *   -> train_pi_iters x { gm_ppo_learner_grad_pi -> the KL stop -> gm_ppo_learner_step_pi }
 *   -> train_vf_iters x { gm_ppo_learner_grad_vf -> gm_ppo_learner_step_vf }
 * the same kernels in the same order as the calls, so every result equals theirs bit for bit.  The
 * stop is the reference's: the first policy iteration whose kl > max_kl_ratio * target_kl takes no
 * step and ends the policy loop; it latches on the device, the later launches are no-ops and the
 * host reads the count of steps taken once, with info (may be NULL).  Advantages and returns live
 * in the learner (grown to n_steps * n_envs floats each on demand). */
int  gm_ppo_learner_update(gm_ppo_learner* l, const gm_ac_traj* traj, int n_steps, gm_ppo_info* info);

/* ---- SAC: squashed Gaussian actor, action replay memory, twin critics and the soft Q target ----
 * The collection side of Agent_SAC (rl/agents/ActorCritic.py) and everything of its
 * optimise_model that is forward-only; the learner follows below ("SAC learner").
 *   actor    h = mlp([n_obs, *hidden], act, act)(obs): the activation follows every hidden Linear;
 *            mu = mu_layer(h), log_std = clamp(log_std_layer(h), log_std_min, log_std_max);
 *            u = mu + exp(log_std) z (GM_SAC_SAMPLE) or u = mu (GM_SAC_MEAN);
 *            logp = sum_i Normal(mu, std).log_prob(u)_i - sum_i 2 (log 2 - u_i - softplus(-2 u_i));
 *            a = action_limit tanh(u)
 *   critics  q_j = mlp([n_obs + n_actions, *hidden, 1], act)(cat(obs, a)), j = 1, 2
 * f32 on the DQN policy's MFMA forward.  The draws are the PPO sampler's counters, keyed by (seed,
 * global env id, decision, action index): c_1, c_2 -> Box-Muller z; c_3 -> the uniform action
 * 2 u3 - 1 of GM_SAC_RANDOM (select_action before random_start_episodes: the net is not used and
 * u, logp, mu, log_std are written as 0).
 * Flat parameter order (torch's parameters() order for MLPActorCriticAC): the actor's hidden
 * layers W0 [out x in], b0, ..., mu_layer.W, b, log_std_layer.W, b, then q1's layers, then q2's. */
#define GM_SAC_MEAN   0
#define GM_SAC_SAMPLE 1
#define GM_SAC_RANDOM 2
typedef struct gm_sac_opt {
  int32_t activation;     /* hidden activation of all three nets: 0 ReLU (default), 1 Tanh */
  float   action_limit;   /* 1 */
  float   log_std_min;    /* -20 */
  float   log_std_max;    /* 2 */
} gm_sac_opt;
void gm_sac_opt_default(gm_sac_opt* out);
/* The transition memory with a float action row; gm_replay's ring rules (row0, the row of env e at
 * env-step k, no row written twice in a call) hold unchanged. */
typedef struct gm_sac_replay {
  int64_t  capacity;    /* rows */
  float*   state;       /* [capacity][n_obs]      observation the action was chosen from */
  float*   action;      /* [capacity][n_actions]  the squashed action the env received (before its clip) */
  float*   next_state;  /* [capacity][n_obs]      observation after the env-step, never the reset one */
  float*   reward;      /* [capacity] */
  uint8_t* end;         /* [capacity]  0 episode continues, 1 terminal (done), 2 truncated only */
} gm_sac_replay;
typedef struct gm_sac_batch {
  float*   state;       /* [batch][n_obs] */
  float*   action;      /* [batch][n_actions] */
  float*   next_state;  /* [batch][n_obs] */
  float*   reward;      /* [batch] */
  uint8_t* end;         /* [batch] */
  int32_t* index;       /* [batch] the ring rows gathered */
} gm_sac_batch;
/* sizeof of 0 gm_sac_replay, 1 gm_sac_batch, 2 gm_sac_opt, 4 gm_sac_learn_opt (-1 otherwise, 3
 * included): for bindings */
int64_t gm_sac_struct_size(int which);
typedef struct gm_sac gm_sac;
/* The device layout of the parameters: [pi | q1 | q2], each net in gm_policy_pack's layout; pi is
 * the one MLP [n_obs, *hidden, 2 n_actions] whose output layer is mu_layer stacked over
 * log_std_layer.  pi_sizes = [n_obs, *hidden, n_actions], q_sizes = [n_obs + n_actions, *hidden, 1].
 * Returns the packed float count (out may be NULL: the count and the offsets only); offsets (may
 * be NULL) receives the float offsets of q1 and q2.  Negative for unsupported sizes: a width above
 * 256, more than 8 layers, n_actions above 40, q_sizes[0] != pi_sizes[0] + n_actions, a critic
 * output other than 1 or an unknown activation.  Host only, no GPU needed. */
int64_t gm_sac_pack(const int32_t* pi_sizes, int n_pi, const int32_t* q_sizes, int n_q, int activation,
                    const float* params, float* out, int64_t* offsets);
/* opt may be NULL (the defaults).  The env must have continuous actions and the actor must map
 * n_obs to n_actions.  A target network (mlp_ac_targ) is a second handle created from the same
 * parameters. */
int  gm_sac_create(gm_ctx* ctx, const int32_t* pi_sizes, int n_pi, const int32_t* q_sizes, int n_q,
                   const gm_sac_opt* opt, const float* params, gm_sac** out);
void gm_sac_destroy(gm_sac* p);
int  gm_sac_set_params(gm_sac* p, const float* params);
int  gm_sac_get_params(gm_sac* p, float* flat);
int  gm_sac_get_packed(gm_sac* p, float* packed);
/* select_action for every env from its current observation (mode: GM_SAC_*), the draws at
 * `decision`.  Keeps act, logp, u, mu and the clamped log_std in the handle's device arrays and
 * applies the actions as gm_ac_act does: clipped to [-1, 1], set in order. */
int  gm_sac_act(gm_sac* p, int mode, uint64_t seed, uint64_t decision);
/* What the last gm_sac_act left: act, u, mu, log_std [n_envs][n_actions], logp [n_envs].  Host
 * pointers; any may be NULL. */
int  gm_sac_read(gm_sac* p, float* act, float* logp, float* u, float* mu, float* log_std);
/* ReplayMemory.push in two halves around gm_step, by gm_policy_push_begin / _end's rules: the same
 * ring row, the same end code, next_state the post-step observation before any reset. */
int  gm_sac_push_begin(gm_sac* p, const gm_sac_replay* replay, int64_t row0);
int  gm_sac_push_end(gm_sac* p, const gm_sac_replay* replay, int64_t row0, int max_episode_steps);
/* The fused rollout.  For k = 0 .. n_steps - 1
 *   gm_sac_act(mode, seed, decision0 + k) -> gm_sac_push_begin(row0 + k * n_envs) -> gm_step
 *   -> gm_sac_push_end(row0 + k * n_envs, max_episode_steps)
 *   -> gm_autoreset_episodes(max_episode_steps, spawn = NULL, records + k * n_envs)
 * as ONE persistent launch of gm_rollout's kind: each env's own wave runs the actor between its
 * env-steps.  State, observations, records and every array of the memory equal the per-step
 * sequence's bit for bit; under GM_CHUNK_SUBSTEPS=0 it runs that sequence.  replay may be NULL
 * (nothing is recorded; row0 is ignored).  records: device [n_steps][n_envs], may be NULL.  The
 * caller advances its count of pushed transitions by n_steps * n_envs. */
int  gm_sac_rollout(gm_sac* p, int n_steps, int mode, uint64_t seed, uint64_t decision0, int max_episode_steps,
                    gm_episode_end* records, const gm_sac_replay* replay, int64_t row0);
/* ReplayMemory.batch: gm_replay_indices' rows (the same keyed bijection) gathered into out's
 * arrays, float action rows included, in one kernel. */
int  gm_sac_replay_sample(gm_ctx* ctx, const gm_sac_replay* replay, int64_t size, int batch, uint64_t seed,
                          uint64_t draw, const gm_sac_batch* out);
/* Both critics on cat(state, action) for n rows: state [n][n_obs], action [n][n_actions] (two
 * independent device arrays), q1, q2: device [n], either may be NULL. */
int  gm_sac_q(gm_sac* p, const float* state, const float* action, int n, float* q1, float* q2);
/* compute_loss_q's backup for the first n rows of a batch, no gradient involved:
 *   a2, logp2 = online's actor on next_state, GM_SAC_SAMPLE, the draws keyed (seed, batch row i as
 *               the id, `draw` as the decision) -- pass a seed other than the rollout's, or batch
 *               row i would repeat env i's exploration noise;
 *   qmin = min(q1, q2) of target's critics on (next_state, a2);
 *   y = reward + gamma (qmin - alpha logp2) where the row bootstraps, y = reward exactly where not.
 * bootstrap_truncated = 0 is the reference as written (no bootstrap where end != 0);
 * bootstrap_truncated = 1 keeps the bootstrap where end == 2.  Reads batch->next_state, reward and
 * end.  y: device [n]; a2, u2 [n][n_actions], logp2, qmin [n]: optional device outputs, any may be
 * NULL.  Two launches (the actor, then the critics) with no host synchronisation between them. */
int  gm_sac_target(gm_sac* target, gm_sac* online, const gm_sac_batch* batch, int n, float gamma, float alpha,
                   int bootstrap_truncated, uint64_t seed, uint64_t draw, float* y, float* a2, float* u2,
                   float* logp2, float* qmin);

/* ---- SAC learner: critic and actor backward, two optimisers and the polyak update ----
 * Agent_SAC.optimise_model (rl/agents/ActorCritic.py:452-500) on the packed device weights
 * [pi | q1 | q2] that gm_sac_rollout reads; no weight crosses the bus.  In the reference's order:
 *   y        = gm_sac_target's backup
 *   loss_q   = mean((q1(o, a) - y)^2) + mean((q2(o, a) - y)^2); q_optimiser steps [q1 | q2]
 *   loss_pi  = mean(alpha logp_pi - min(q1, q2)(o, pi(o))) with the critics as that step left them,
 *              frozen (none of their weight gradients is formed), and fresh noise; pi_optimiser
 *              steps [pi].  A tie of the min goes to q1.
 *   polyak   theta_targ <- (1 - tau) theta_targ + tau theta over all three nets.
 * Optimisers as Agent_SAC.init builds them: "adam" is torch.optim.Adam(lr, betas); "adamW" is
 * torch.optim.AdamW(lr, betas, amsgrad=True) with torch's weight_decay 0.01.  No gradient clamp.
 * The reference hands pi_optimiser all of mlp_ac.parameters() under AdamW, but the critics' .grad
 * is None when it steps (zero_grad sets None under torch >= 2.0), so it skips them, decay
 * included: here pi_optimiser owns [pi] alone.  RMSprop is not on the device. */
typedef struct gm_sac_learn_opt {   /* doubles, as torch keeps its hyperparameters */
  int32_t optimiser;                /* GM_OPT_ADAM (default) / GM_OPT_ADAMW */
  int32_t amsgrad;
  double  lr, beta1, beta2, eps, weight_decay;
} gm_sac_learn_opt;
/* Agent_SAC.Parameters' defaults: Adam, lr 1e-4, betas (0.9, 0.999), eps 1e-8, no decay, no amsgrad */
void gm_sac_learn_opt_default(gm_sac_learn_opt* out);
/* A learner for `online`, on its context: owns the per-tile partial gradients, both summed
 * gradients, exp_avg / exp_avg_sq / max_exp_avg_sq of both optimisers (zero), their step counts (0)
 * and the scratch, sized for batches of up to GM_LEARNER_MAX_BATCH rows.  Destroy it before `online`. */
typedef struct gm_sac_learner gm_sac_learner;
int  gm_sac_learner_create(gm_sac* online, const gm_sac_learn_opt* opt, gm_sac_learner** out);
void gm_sac_learner_destroy(gm_sac_learner* l);
/* loss_q.backward() for the first n rows of a batch (state and action are read) and the backup y
 * (device [n]): leaves the raw gradient of [q1 | q2] and loss_q on the device.
 * n > GM_LEARNER_MAX_BATCH is GM_E_ARG. */
int  gm_sac_learner_grad_q(gm_sac_learner* l, const gm_sac_batch* batch, const float* y, int n);
/* loss_pi.backward() for the first n rows of a batch (state is read): row i draws with (seed, i,
 * draw), gm_sac_target's keys.  Leaves the raw gradient of [pi] and loss_pi on the device; the
 * critics' held gradient is untouched.  z, u, a: [n][n_actions], logp, q1, q2: [n]: optional
 * device outputs (the draws, the pre-squash sample, the action, its log-probability and both
 * critics on it), any may be NULL. */
int  gm_sac_learner_grad_pi(gm_sac_learner* l, const gm_sac_batch* batch, int n, float alpha, uint64_t seed,
                            uint64_t draw, float* z, float* u, float* a, float* logp, float* q1, float* q2);
/* q_optimiser.step() / pi_optimiser.step() on the held gradient, in place on the online handle's
 * device weights: [q1 | q2] alone / [pi] alone.  That optimiser's step count goes up by one. */
int  gm_sac_learner_step_q(gm_sac_learner* l);
int  gm_sac_learner_step_pi(gm_sac_learner* l);
/* target <- tau online + (1 - tau) target over the whole blob (ActorCritic.py:494-500); the two
 * handles need the same sizes and context.  The sum is formed in double and rounded once; tau = 1
 * copies online bit for bit. */
int  gm_sac_soft_update(gm_sac* target, gm_sac* online, float tau);
/* Both held gradients in gm_sac_create's flat order (one array: [pi | q1 | q2]), loss_q and
 * loss_pi (host pointers; any may be NULL). */
int  gm_sac_learner_read(gm_sac_learner* l, float* grad_flat, float* loss_q, float* loss_pi);
/* Both optimisers' state_dict() tensors in flat order (one array each: the [q1 | q2] part is
 * q_optimiser's, the [pi] part pi_optimiser's); steps: [2] = q_optimiser's, pi_optimiser's.  Host
 * pointers; any may be NULL. */
int  gm_sac_learner_get_state(gm_sac_learner* l, int64_t* steps, float* exp_avg, float* exp_avg_sq,
                              float* max_exp_avg_sq);
int  gm_sac_learner_set_state(gm_sac_learner* l, const int64_t* steps, const float* exp_avg, const float* exp_avg_sq,
                              const float* max_exp_avg_sq);
/* n_updates of optimise_model enqueued with no host synchronisation between them: for u = 0 ..
 * n_updates - 1, with d = draw0 + u,
 *   gm_sac_replay_sample(size, batch, seed, d) into the learner's own batch arrays
 *   -> gm_sac_target(target, online, gamma, alpha, bootstrap_truncated, noise_seed, 2 d)
 *   -> gm_sac_learner_grad_q -> gm_sac_learner_step_q
 *   -> gm_sac_learner_grad_pi(alpha, noise_seed, 2 d + 1) -> gm_sac_learner_step_pi
 *   -> gm_sac_soft_update(target, online, tau)
 * every result equal to the calls' bit for bit (each range's polyak update rides in that range's
 * step launch, which is elementwise the same).  tau <= 0 skips the polyak update.  losses: device
 * [n_updates][2] (loss_q, loss_pi of every update) or NULL. */
int  gm_sac_learner_train(gm_sac_learner* l, gm_sac* target, const gm_sac_replay* replay, int64_t size, int batch,
                          uint64_t seed, uint64_t noise_seed, uint64_t draw0, int n_updates, float gamma, float alpha,
                          int bootstrap_truncated, float tau, float* losses);

/* ---- batched evaluation: one test episode per env, then the env retires (DESIGN.md §5,
 * "Evaluation launch") ----
 * MujocoTrainer.test() runs every test episode to its end and keeps MjEnv._monitor_test's
 * test report of it (the cumulative reward and the event track).  An evaluation launch does that
 * for every active env at once: each runs from its current state until its episode ends
 * (gm_episode_end_code: 1 done, 2 truncated at num_action_steps >= max_episode_steps, so at
 * most max_episode_steps env-steps wherever the env started), writes its report and leaves the
 * work queue; the launch ends with the last episode.  Nothing is reset and nothing is recorded
 * into a trajectory buffer or a replay memory.
 *
 * The report, device arrays, one row per env (W = binary + linear events in gm_get_event_rows'
 * column order): what gm_get_event_rows and the state record hold at the episode's last
 * env-step before any reset, i.e. MjClass::get_test_report plus MjEnv.track.cumulative_reward.
 * An inactive env gets end = 0 and its other rows are not touched. */
typedef struct gm_eval_out {
  float*   ret;      /* [n_envs] cumulative_reward at the episode's end                        */
  int32_t* length;   /* [n_envs] num_action_steps at the end                                   */
  uint8_t* end;      /* [n_envs] gm_episode_end_code (1 done, 2 truncated); 0: env not active  */
  int32_t* rows;     /* [n_envs x W]                                                           */
  int32_t* abs;      /* [n_envs x W]                                                           */
  float*   last;     /* [n_envs x W]                                                           */
} gm_eval_out;
/* The per-step half: after a gm_step, every env with active_inout[e] != 0 whose episode has ended
 * writes its report and clears its active byte (active_inout: device [n_envs], required).  With
 * it the evaluation launches below have the per-step sequence every fused launch here has,
 *   act -> gm_step -> gm_eval_record -> gm_autoreset_episodes(max_episode_steps, spawn = NULL),
 * max_episode_steps times: envs that have reported carry on into later episodes and are ignored.
 * Envs are independent, so the reports are bit for bit the fused launch's; that sequence is also
 * what the entry points run when the queue is off (GM_CHUNK_SUBSTEPS=0), on a private copy of
 * active (the caller's array is never written by them), after setting end = 0 for every inactive env. */
int  gm_eval_record(gm_ctx* ctx, int max_episode_steps, uint8_t* active_inout, const gm_eval_out* out);
/* The evaluation launches.  active: device [n_envs] bytes, NULL = every env.  out: every array
 * required.  max_episode_steps <= 0 (the launch would be unbounded), a NULL out or a missing
 * array are GM_E_ARG with a gm_last_error text, and nothing is launched.
 *   gm_evaluate         the scripted drivers, params->action_mode 0, 1, 3 or 4 (3, the grasp
 *                       program, is Trainer.test(heuristic=True)); params->max_episode_steps bounds it
 *   gm_policy_evaluate  the DQN policy, greedy (eps = 0)
 *   gm_ac_evaluate      both actor kinds; sample = 1 is the reference's PPO test mode, which still
 *                       samples (noise is 0), sample = 0 the mean / the argmax.  The actor-critic
 *                       handle owns the one-row scratch trajectory the actor's phases write into
 *   gm_sac_evaluate     mode GM_SAC_MEAN is the test mode; GM_SAC_SAMPLE / GM_SAC_RANDOM are accepted
 * An agent's handle needs the action kind it was created for: the creators refuse the other kind,
 * and where gm_update_config has changed continous_actions since, the three agent calls return
 * GM_E_ARG with a gm_last_error text and launch nothing.  A NULL handle is GM_E_ARG.
 * An inactive env shows in the launch's diagnostics as a job of 0 clocks and 0 yields
 * (gm_chunk_job_stats) that finished at the moment it was picked (gm_chunk_timeline).
 * The reports are a deterministic function of the env states and the arguments at the call.  The
 * env state after the call is NOT specified beyond that: the fused launch leaves every active env
 * parked at its terminal state (episode not advanced, num_action_steps = length), the per-step
 * sequence leaves it somewhere in a later episode.  Reset before reuse (gm_reset).
 * gm_last_step_ms then times the whole launch, and its per-env-step divisor, gm_dispatch_info
 * out[3], is max_episode_steps: an upper bound of the env-steps an env ran, so ms / out[3] is a
 * lower bound of the time per env-step; for envs that started at a reset, out->length summed over
 * the active envs is the number of env-steps the launch ran. */
int  gm_evaluate(gm_ctx* ctx, const gm_rollout_params* params, const uint8_t* active, const gm_eval_out* out);
int  gm_policy_evaluate(gm_policy* p, uint64_t seed, uint64_t decision0, int max_episode_steps, const uint8_t* active,
                        const gm_eval_out* out);
int  gm_ac_evaluate(gm_ac* p, int sample, uint64_t seed, uint64_t decision0, int max_episode_steps,
                    const uint8_t* active, const gm_eval_out* out);
int  gm_sac_evaluate(gm_sac* p, int mode, uint64_t seed, uint64_t decision0, int max_episode_steps,
                     const uint8_t* active, const gm_eval_out* out);

#ifdef __cplusplus
}
#endif

#endif /* GRIPPER_MI355X_H_ */
