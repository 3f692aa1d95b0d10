// gm_capi.hip -- C ABI (include/gripper_mi355x.h) over the device kernels.
//
// Replaces the pybind11 MjClass boundary (src/bind.cpp:43-205).  A context owns
// one HIP stream and the device buffers of n_envs envs; every call is
// asynchronous on that stream except the host-buffer getters, which copy and
// synchronise.  No C++ exception crosses the ABI: failures return GM_E_* and
// leave a message for gm_last_error().
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include <mutex>

#include "gm_kernels.hip"
#include "gm_env_kernels.hip"
#include "gm_policy.hip"
#include "gm_replay.hip"
#include "gm_learn.hip"
#include "gm_ac.hip"
#include "gm_ppo_learn.hip"
#include "gm_sac.hip"
#include "gm_sac_learn.hip"

// calibration translation unit (gm_calib.hip)
hipError_t gm_cal_launch_step(int n_seg, int n_envs, hipStream_t st, GmEnvState* states, const gm_model* m,
                              const gm_config* C, const GmTopo* T);
hipError_t gm_cal_launch_setup(hipStream_t st, GmEnvState* states, const double* dt, const int32_t* steps, double tip,
                               int n);
hipError_t gm_cal_launch_read(hipStream_t st, const GmEnvState* states, uint8_t* bad, int n);
hipError_t gm_cal_launch_gauge(int n_seg, hipStream_t st, const GmEnvState* states, const gm_model* m, const GmTopo* T,
                               int env, float* out);

// evaluation translation unit (gm_eval.hip): the evaluation launch's kernel instantiations
hipError_t gm_eval_launch_step(int n_seg, bool duo, int grid, hipStream_t st, GmEnvState* states, const gm_model* m,
                               const gm_config* C, const GmTopo* T, float* obs, float* rew, uint8_t* done, int n_envs,
                               const int32_t* order, uint32_t* cost, const GmChunkQ& q);

// Move-only owner of one hipMalloc allocation of T (Pinned: of one hipHostMalloc allocation): the
// only code of this file that allocates or frees device or pinned memory.  It reads as the raw
// pointer wherever one is expected; a copy of that pointer is a view and frees nothing.
template <class T, bool Pinned = false>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
    return *this;
  }
  ~DevBuf() { reset(); }
  // n elements, uninitialised; what the owner held before is released first
  hipError_t alloc(size_t n) {
    reset();
    return Pinned ? hipHostMalloc(&p_, sizeof(T) * n, hipHostMallocDefault) : hipMalloc(&p_, sizeof(T) * n);
  }
  void reset() {
    if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));   // (hipFree synchronises the whole device)
    p_ = nullptr;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }

 private:
  T* p_ = nullptr;
};
template <class T>
using HostBuf = DevBuf<T, true>;

struct gm_ctx {
  int device = 0;
  int n_envs = 0;
  long long env_offset = 0;
  int n_objects = 0;
  hipStream_t stream = nullptr;        // stream every launch of this ctx goes to
  hipStream_t own_stream = nullptr;    // the one gm_create made (destroyed with the ctx)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  int last_launch_steps = 1;           // env-steps per env of the last timed launch
  gm_model model;
  gm_config cfg;
  GmTopo topo;
  // device buffers: every DevBuf / HostBuf is released with the context (gm_destroy, after
  // its last synchronise); the raw pointers among them are views
  DevBuf<GmEnvState> d_state;
  DevBuf<gm_model> d_model;
  DevBuf<gm_config> d_cfg;
  DevBuf<GmTopo> d_topo;
  DevBuf<gm_object> d_objs;
  DevBuf<double> d_eq;
  float* d_obs = nullptr;              // d_obs, d_rew, d_done: views into one allocation (d_out),
  float* d_rew = nullptr;              // read back by gm_get_outputs in one copy through h_out
  uint8_t* d_done = nullptr;           // (pinned)
  DevBuf<char> d_out;
  HostBuf<char> h_out;
  size_t out_bytes = 0;
  DevBuf<float> d_act;
  // host actions are staged through a pinned buffer so gm_set_action / gm_set_discrete_action
  // return without a stream synchronisation (stage_ev: the previous staging copy is done)
  HostBuf<char> h_stage;
  size_t stage_bytes = 0;
  hipEvent_t stage_ev = nullptr;
  DevBuf<int32_t> d_dact;
  DevBuf<uint8_t> d_mask;
  DevBuf<uint8_t> d_eval_active;       // the per-step evaluation's working copy of the caller's active bytes
  // scratch of the force-measurement calls (gm_set_motor_target's targets and flags,
  // gm_get_sensor_si's readings): allocated once with the context, no per-call allocation
  // (freeing one synchronises the whole device)
  DevBuf<char> d_scratch;
  DevBuf<gm_spawn> d_spawn;
  DevBuf<int32_t> d_order;             // workgroup -> env dispatch order (cost-sorted)
  DevBuf<uint32_t> d_cost;             // per-env cost of the last env-step (clocks / 64)
  // chunked env-step (gm_step_chunked_kernel): queue counters, per-XCD continuation rings,
  // per-env carry; chunk = substeps per chunk (0: the one-shot kernel)
  DevBuf<uint32_t> d_chunk_ctr;
  DevBuf<uint64_t> d_chunk_ring;
  DevBuf<GmChunkCarry> d_chunk_carry;
  DevBuf<unsigned long long> d_chunk_st;
  int chunk = 0, chunk_grid = 0, chunk_cap = 0, chunk_margin = 50, chunk_yields = 20, chunk_cmargin = 50;
  int chunk_steal = 1;                 // idle waves resume yielded envs of other XCDs (GM_CHUNK_STEAL=0: off)
  int chunk_prio = 1;                  // issue priority by predicted work left (GM_CHUNK_PRIO=0: off)
  // DUO workgroups (gm_step_kernel<CL, false, true>): two waves per env, the second running
  // the collider concurrently -- for batches small enough that wave slots are spare
  bool duo = false;
  DevBuf<gm_spawn_params> d_scene;     // gm_set_scene_spawn parameters (empty: plain spawn_object)
  int scene_tries = 0;
  GmSpawnRand spawn_rand{};            // gm_set_random_spawn (enable = 0: spawn tables)
  std::string err;
};

namespace {

int fail(gm_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}
#define HIPCHK(ctx, x)                                                               \
  do {                                                                               \
    hipError_t e_ = (x);                                                             \
    if (e_ != hipSuccess)                                                            \
      return fail(ctx, GM_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_));    \
  } while (0)

// host bytes -> device, owned by the stream before the call returns: through the context's
// pinned staging buffer (stage_ev: its previous copy has left it), or copy and wait
static int stage_upload(gm_ctx* c, void* dst, const void* src, size_t bytes) {
  if (bytes <= c->stage_bytes) {
    HIPCHK(c, hipEventSynchronize(c->stage_ev));
    std::memcpy(c->h_stage, src, bytes);
    HIPCHK(c, hipMemcpyAsync(dst, c->h_stage, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->stage_ev, c->stream));
  } else {
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return GM_OK;
}
// a thread-per-env kernel on the context's stream
template <class K, class... A>
hipError_t launch_per_env(const gm_ctx* c, K kernel, const A&... args) {
  const int threads = 64, blocks = (c->n_envs + threads - 1) / threads;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, c->stream, args...);
  return hipGetLastError();
}
// the caller's per-env mask on the device (dm; NULL without one: every env)
hipError_t upload_mask(gm_ctx* c, const uint8_t* mask, const uint8_t*& dm) {
  dm = mask ? c->d_mask.get() : nullptr;
  return mask ? hipMemcpyAsync(c->d_mask, mask, (size_t)c->n_envs, hipMemcpyHostToDevice, c->stream) : hipSuccess;
}
// a device range to the caller's array (host, or device with on_device), complete on return
int read_back(gm_ctx* c, void* dst, const void* src, size_t bytes, int on_device = 0) {
  HIPCHK(c, hipMemcpyAsync(dst, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GM_OK;
}
// gm_reset_kernel: one 64-lane workgroup per env, the envs of the device mask dm (NULL: all),
// poses from the device table ds (NULL: the context's spawn rule)
hipError_t launch_reset(gm_ctx* c, const uint8_t* dm, const gm_spawn* ds) {
  hipLaunchKernelGGL(gm_reset_kernel, dim3(c->n_envs), dim3(64), 0, c->stream, c->d_state, c->d_model, c->d_cfg,
                     c->d_topo, c->d_eq, dm, ds, c->d_objs, c->n_objects, c->n_envs, c->d_scene, c->scene_tries,
                     c->d_obs, c->spawn_rand);
  return hipGetLastError();
}

bool nseg_supported(int n) {
  switch (n) {
#define X(N) case N:
    GM_NSEG_LIST
#undef X
    return true;
    default: return false;
  }
}
// job: a rollout's (rollout_job; it needs the chunked queue), NULL: one plain env-step per env;
// eval: the job is an evaluation's (eval_launch), run by gm_eval.hip's instantiations
hipError_t launch_step(gm_ctx* c, int grid, int n_envs, int mode, DebugOut dbg, const GmRolloutJob* job = nullptr,
                       bool eval = false) {
  // the full env-step (mode 0) runs in cost-sorted order and records each env's cost
  const int32_t* order = (mode == 0 && grid == c->n_envs) ? c->d_order.get() : nullptr;
  uint32_t* cost = (mode == 0 && grid == c->n_envs) ? c->d_cost.get() : nullptr;
  // the chunked work queue (gm_chunkq.h, gm_rollout.h chunked_env_steps): one workgroup per
  // resident wave slot, each pulling env chunks until every env has finished
  const bool chunked = order && c->chunk > 0 && c->chunk_grid > 0 && dbg.phase == nullptr;
  GmChunkQ q{c->d_chunk_ctr, c->d_chunk_ring, c->d_chunk_carry, c->chunk_cap, chunked ? c->chunk : 0,
             c->chunk_margin, c->chunk_yields, c->chunk_cmargin, c->d_chunk_st, c->chunk_steal, c->chunk_prio};
  q.job.steps = 1;
  q.job.driver = GM_DRV_NONE;
  if (job && chunked) q.job = *job;
  if (chunked) grid = c->chunk_grid;
  // the env-step proper (not the settle, a diagnostic substep or a profiled step) on DUO
  // workgroups when the context chose them; the chunked grid was sized for that kernel
  const bool duo = c->duo && mode == 0;   // (a profiled step too: the owner wave's phase clocks)
  if (eval)
    return job && chunked ? gm_eval_launch_step(c->model.n_seg, duo, grid, c->stream, c->d_state, c->d_model, c->d_cfg,
                                                c->d_topo, c->d_obs, c->d_rew, c->d_done, n_envs, order, cost, q)
                          : hipErrorInvalidValue;
  switch (c->model.n_seg) {
#define X(N)                                                                                                 \
  case N:                                                                                                    \
    if (duo)                                                                                                 \
      hipLaunchKernelGGL((gm_step_kernel<N + 2, false, true>), dim3(grid), dim3(2 * NT), 0, c->stream,        \
                         c->d_state, c->d_model, c->d_cfg, c->d_topo, c->d_obs, c->d_rew, c->d_done, n_envs,   \
                         mode, dbg, order, cost, q);                                                           \
    else                                                                                                     \
      hipLaunchKernelGGL((gm_step_kernel<N + 2, false>), dim3(grid), dim3(NT), 0, c->stream, c->d_state,      \
                         c->d_model, c->d_cfg, c->d_topo, c->d_obs, c->d_rew, c->d_done, n_envs, mode, dbg,    \
                         order, cost, q);                                                                      \
    return hipGetLastError();
    GM_NSEG_LIST
#undef X
    default: return hipErrorInvalidValue;
  }
}
// The timed env-step launch (gm_step, and the rollouts' one persistent launch of job->steps
// env-steps per env) and the next launch's dispatch order
int timed_launch(gm_ctx* c, const GmRolloutJob* job, bool eval = false) {
  DebugOut dbg{nullptr, nullptr, nullptr, nullptr, nullptr};
  HIPCHK(c, hipEventRecord(c->ev0, c->stream));
  HIPCHK(c, launch_step(c, c->n_envs, c->n_envs, 0, dbg, job, eval));
  HIPCHK(c, hipEventRecord(c->ev1, c->stream));
  hipLaunchKernelGGL(gm_dispatch_order_kernel, dim3(1), dim3(1024), 0, c->stream, c->d_cost, c->d_order, c->n_envs,
                     c->d_chunk_ctr, c->d_chunk_st);
  HIPCHK(c, hipGetLastError());
  c->timed = true;
  c->last_launch_steps = job ? job->steps : 1;
  return GM_OK;
}
// A rollout entry point runs as one persistent launch of a rollout_job when the queue is on ...
bool chunk_queue_on(const gm_ctx* c) { return c->chunk > 0 && c->chunk_grid > 0; }
GmRolloutJob rollout_job(const gm_ctx* c, int steps, GmDriver driver, uint64_t seed, float jitter, int max_ep,
                         gm_episode_end* rec) {
  GmRolloutJob j{steps, driver, seed, jitter, max_ep, rec, c->d_eq, c->d_objs, c->n_objects, c->scene_tries,
                 c->d_scene, c->spawn_rand};
  j.sr.env_offset = c->env_offset;   // (the driver's global env ids even without random spawns)
  return j;
}
// ... and with the one-shot kernel (GM_CHUNK_SUBSTEPS=0) as the per-step sequence the launch
// fuses: the driver's before(k) -> gm_step -> its after(k) -> gm_autoreset_episodes
template <class Before, class After>
int per_step_rollout(gm_ctx* c, int n_steps, int max_ep, gm_episode_end* records, Before before, After after) {
  for (int k = 0; k < n_steps; k++) {
    int rc = before(k);
    if (rc == GM_OK) rc = gm_step(c);
    if (rc == GM_OK) rc = after(k);
    if (rc == GM_OK) rc = gm_autoreset_episodes(c, max_ep, nullptr, 1, nullptr,
                                                records ? records + (size_t)k * c->n_envs : nullptr);
    if (rc != GM_OK) return rc;
  }
  return GM_OK;
}
// An agent's evaluation needs the action kind its handle was created for (gm_policy_create's,
// gm_ac_create's and gm_sac_create's rule, here for a config that gm_update_config changed since:
// the network's outputs would no longer be the env's actions)
int eval_action_kind(gm_ctx* c, const char* who, bool continuous, const char* agent) {
  if ((c->cfg.s.continous_actions != 0) == continuous) return GM_OK;
  return fail(c, GM_E_ARG, std::string(who) + ": " + agent + " needs " + (continuous ? "continuous" : "discrete") +
                               " actions (continous_actions " + (continuous ? "!= 0)" : "= 0)"));
}
// An evaluation entry point (gm_evaluate and the like; who: its name): the checks they share ...
int eval_check(gm_ctx* c, const char* who, int max_ep, const gm_eval_out* out) {
  if (max_ep <= 0)
    return fail(c, GM_E_ARG, std::string(who) + ": max_episode_steps must be positive (the launch would be unbounded)");
  if (!out || !out->ret || !out->length || !out->end || !out->rows || !out->abs || !out->last)
    return fail(c, GM_E_ARG, std::string(who) + ": no report arrays, or one of ret, length, end, rows, abs, last missing");
  return GM_OK;
}
// ... the job as one persistent launch when the queue is on: every active env runs until its
// episode ends (at most job.steps = max_episode_steps env-steps), reports and retires ...
int eval_launch(gm_ctx* c, GmRolloutJob job, const uint8_t* active, const gm_eval_out* out) {
  job.rec = nullptr;
  job.active = active;
  job.ev = *out;
  return timed_launch(c, &job, true);
}
hipError_t launch_eval_record(gm_ctx* c, int max_ep, uint8_t* active, const gm_eval_out* out, int init) {
  hipLaunchKernelGGL(gm_eval_record_kernel, dim3(c->n_envs), dim3(64), 0, c->stream, c->d_state.get(), c->d_done,
                     max_ep, active, *out, c->n_envs, init);
  return hipGetLastError();
}
// ... and with the one-shot kernel as the per-step sequence the launch fuses, max_ep times: the
// driver's before(k) -> gm_step -> gm_eval_record -> gm_autoreset_episodes, on the context's own
// copy of the active bytes (envs that have reported carry on into later episodes, ignored)
template <class Before>
int per_step_evaluate(gm_ctx* c, int max_ep, const uint8_t* active, const gm_eval_out* out, Before before) {
  if (active)
    HIPCHK(c, hipMemcpyAsync(c->d_eval_active, active, (size_t)c->n_envs, hipMemcpyDeviceToDevice, c->stream));
  else
    HIPCHK(c, hipMemsetAsync(c->d_eval_active, 1, (size_t)c->n_envs, c->stream));
  HIPCHK(c, launch_eval_record(c, max_ep, c->d_eval_active, out, 1));
  for (int k = 0; k < max_ep; k++) {
    int rc = before(k);
    if (rc == GM_OK) rc = gm_step(c);
    if (rc != GM_OK) return rc;
    HIPCHK(c, launch_eval_record(c, max_ep, c->d_eval_active, out, 0));
    rc = gm_autoreset_episodes(c, max_ep, nullptr, 1, nullptr, nullptr);
    if (rc != GM_OK) return rc;
  }
  return GM_OK;
}

int build_topo(const gm_model& m, GmTopo& T, std::string& err) {
  std::memset(&T, 0, sizeof(T));
  T.N = m.n_seg;
  T.CL = m.n_seg + 2;
  T.nbody = m.nbody; T.nv = m.nv; T.nq = m.nq; T.ngeom = m.ngeom; T.npair = m.npair; T.nlock = m.nlock;
  T.body_base = m.body_base; T.dof_base = m.dof_base;
  for (int f = 0; f < 3; f++) {
    T.dof_f0[f] = m.dof_pris[f];
    T.body_f0[f] = m.dof_body[m.dof_pris[f]];
    T.body_finger[f] = m.body_finger[f];
  }
  T.body_palm = m.body_palm; T.dof_palm = m.dof_palm;
  T.body_obj = m.body_obj; T.dof_obj = m.dof_obj; T.geom_obj = m.geom_obj;
  T.qadr_obj = m.jnt_qposadr[m.body_jnt[m.body_obj]];
  // verify the canonical tree layout the kernels index arithmetically
  for (int f = 0; f < 3; f++)
    for (int p = 1; p <= T.CL; p++) {
      int d = T.dof_f0[f] + p - 1, b = T.body_f0[f] + p - 1;
      if (m.dof_body[d] != b || m.body_group[b] != f) { err = "model is not the canonical gripper tree"; return GM_E_ARG; }
      int par = (p == 1) ? m.dof_base : d - 1;
      if (m.dof_parent[d] != par) { err = "unexpected dof parent"; return GM_E_ARG; }
    }
  if (m.npair > GM_MAX_PAIR || m.npair > NT * gm_pair_batches(T.CL) || m.nv > GM_MAX_DOF || T.qadr_obj != m.dof_obj) {
    err = "model exceeds kernel limits";
    return GM_E_RANGE;
  }
  for (int b = 0; b < GM_MAX_BODY; b++) { T.body_group[b] = -1; T.body_cpos[b] = 0; }
  for (int b = 0; b < m.nbody; b++) {
    T.body_group[b] = m.body_group[b];
    if (m.body_group[b] >= 0 && m.body_group[b] < 3) T.body_cpos[b] = b - T.body_f0[m.body_group[b]] + 1;
    else if (m.body_group[b] == GM_GRP_PALM) T.body_cpos[b] = 1;
  }
  for (int l = 0; l < 64; l++) T.lane_body[l] = -1;
  if (T.CL > 15) { err = "finger chain longer than a 16-lane DPP row"; return GM_E_RANGE; }
  for (int f = 0; f < 3; f++)
    for (int p = 1; p <= T.CL; p++) T.lane_body[16 * f + p] = T.body_f0[f] + p - 1;
  T.lane_base = GM_LANE_BASE;
  T.lane_body[GM_LANE_BASE] = T.body_base;
  T.lane_body[GM_LANE_BASE + 1] = T.body_palm;
  T.lane_body[GM_LANE_BASE + 2] = T.body_obj;
  for (int l = GM_OBJ_LANE0; l < GM_OBJ_LANE0 + 6; l++)   // (gm_shared.h asserts the layout)
    if (T.lane_body[l] >= 0) { err = "a body's scan lane on the object's component lanes"; return GM_E_RANGE; }
  // per-dof constants: the engine-spec H~ diagonal additions and PD gains
  // (mj_step2 implicit damping / PD terms and luke::control gains, oracle.c ctrl_gains / step2)
  for (int d = 0; d < m.nv; d++) {
    const int b = m.dof_body[d], j = m.body_jnt[b];
    T.dof_body[d] = b;
    T.dof_grp[d] = m.body_group[b];
    T.dof_p[d] = (m.body_group[b] == GM_GRP_OBJECT) ? d - m.dof_obj : T.body_cpos[b];
    double kp = 0, kd = 0;
    int tgt = 0;
    for (int f = 0; f < 3; f++) {
      if (d == m.dof_pris[f]) { kp = m.kp_gripper[0]; kd = m.kd_gripper[0]; tgt = 1; }
      if (d == m.dof_rev[f]) { kp = m.kp_gripper[1]; kd = m.kd_gripper[1]; tgt = 2; }
    }
    if (d == m.dof_palm) { kp = m.kp_gripper[2]; kd = m.kd_gripper[2]; tgt = 3; }
    if (d == m.dof_base) { kp = m.kp_base[2]; kd = m.kd_base[2]; tgt = 4; }
    const bool free = m.jnt_type[j] == GM_JNT_FREE;
    // the constraint solve's matrix: M + armature under MuJoCo's actuator order (the PD
    // forces explicit, the joint damping implicit in the Euler step, integrate); with the
    // folded scheme also h (damping + kd) + h^2 kp.  Joint springs are explicit either way.
    const bool mj = m.mujoco_actuators != 0;
    double add = m.jnt_armature[j] + (mj ? 0.0 : m.timestep * (m.jnt_damping[j] + kd));
    if (!free && !mj) add += m.timestep * m.timestep * kp;
    T.dof_add[d] = add;
    T.dof_arm[d] = m.jnt_armature[j];
    T.dof_dsum[d] = mj ? 0.0 : m.jnt_damping[j] + kd;
    T.dof_ksum[d] = (free || mj) ? 0.0 : kp;
    T.dof_stiff[d] = free ? 0.0 : m.jnt_stiffness[j];
    T.dof_damp[d] = m.jnt_damping[j];
    T.dof_kp[d] = kp; T.dof_kd[d] = kd; T.dof_target[d] = tgt;
  }
  for (int g = 0; g < m.ngeom; g++) {
    int b = m.geom_body[g];
    T.geom_group[g] = (b == 0) ? -1 : T.body_group[b];
    if (T.geom_group[g] == GM_GRP_BASE) T.geom_group[g] = -1;
    T.geom_cpos[g] = T.body_cpos[b];
  }
  // flattened per-lane constants (GmTopo kl_* / dof_* / pr_* / lock_*): the same values
  // the kernels read through the model's index chains, resolved here once
  for (int l = 0; l < 64; l++) {
    const int b = T.lane_body[l];
    T.kl_type[l] = -1; T.kl_qadr[l] = 0;
    T.kl_grp[l] = (b >= 0) ? T.body_group[b] : -1;
    const bool chain = T.kl_grp[l] >= 0 && T.kl_grp[l] <= 3;
    T.kl_cpos[l] = chain ? T.body_cpos[b] : 0;
    for (int k = 0; k < 3; k++) { T.kl_pos[l][k] = 0; T.kl_axis[l][k] = 0; }
    T.kl_quat[l][0] = 1; T.kl_quat[l][1] = T.kl_quat[l][2] = T.kl_quat[l][3] = 0;
    if (b > 0) {
      for (int k = 0; k < 3; k++) T.kl_pos[l][k] = m.body_pos[b][k];
      for (int k = 0; k < 4; k++) T.kl_quat[l][k] = m.body_quat[b][k];
      const int j = m.body_jnt[b];
      if (j >= 0) {
        T.kl_type[l] = m.jnt_type[j];
        T.kl_qadr[l] = m.jnt_qposadr[j];
        for (int k = 0; k < 3; k++) T.kl_axis[l][k] = m.jnt_axis[j][k];
      }
    }
  }
  for (int d = 0; d < m.nv; d++) {
    const int j = m.body_jnt[m.dof_body[d]];
    T.dof_jtype[d] = m.jnt_type[j];
    T.dof_k[d] = d - m.jnt_dofadr[j];
    for (int k = 0; k < 3; k++) T.dof_axis[d][k] = m.jnt_axis[j][k];
  }
  for (int p = 0; p < m.npair; p++) {
    const int gs[2] = {m.pair_a[p], m.pair_b[p]};
    for (int s = 0; s < 2; s++) {
      const int g = gs[s];
      T.pr_g[p][s] = g;
      T.pr_type[p][s] = (g == m.geom_obj) ? -1 : m.geom_type[g];
      T.pr_body[p][s] = m.geom_body[g];
      for (int k = 0; k < 3; k++) { T.pr_pos[p][s][k] = m.geom_pos[g][k]; T.pr_size[p][s][k] = m.geom_size[g][k]; }
      for (int k = 0; k < 4; k++) T.pr_quat[p][s][k] = m.geom_quat[g][k];
      T.pr_rbound[p][s] = m.geom_rbound[g];
      T.pr_fric[p][s] = m.geom_friction[g];
    }
  }
  for (int k = 0; k < m.nlock; k++) {
    const int b = m.dof_body[m.lock_dof[k]];
    T.lock_grp[k] = T.body_group[b];
    T.lock_cpos[k] = T.body_cpos[b];
    T.lock_tran[k] = m.body_invweight0[b][0] + m.body_invweight0[m.body_parent[b]][0];
  }
  // per scan lane: the lane body's pairs with the object / the ground (oracle topo_init)
  T.lane_obj = 50;
  T.pair_gobj = -1;
  for (int l = 0; l < 64; l++)
    for (int s = 0; s < 2; s++) { T.lane_opair[l][s] = -1; T.lane_gpair[l][s] = -1; }
  for (int pr = 0; pr < m.npair; pr++) {
    const int a = m.pair_a[pr], bg = m.pair_b[pr];
    const bool with_obj = a == m.geom_obj || bg == m.geom_obj;
    const bool with_gnd = a == m.geom_ground || bg == m.geom_ground;
    if (with_obj && with_gnd) {
      if (T.pair_gobj >= 0) { err = "more than one object-ground pair"; return GM_E_RANGE; }
      T.pair_gobj = pr;
      continue;
    }
    if (!with_obj && !with_gnd) { err = "gripper self-collision pairs are not supported"; return GM_E_RANGE; }
    const int g = with_obj ? (a == m.geom_obj ? bg : a) : (a == m.geom_ground ? bg : a);
    const int b = m.geom_body[g];
    bool assigned = false;
    for (int l = 0; l < 64; l++) {
      if (T.lane_body[l] != b || l == T.lane_obj) continue;
      int32_t* slot = with_obj ? T.lane_opair[l] : T.lane_gpair[l];
      if (slot[0] < 0) slot[0] = pr;
      else if (slot[1] < 0) slot[1] = pr;
      else { err = "a body has more than two object (or ground) pairs"; return GM_E_RANGE; }
      assigned = true;
    }
    // the Newton Hessian composites reach a contact only through its gripper body's scan
    // lane: a pair on a body without one would be solved with an inconsistent Hessian
    if (!assigned) {
      err = "contact pair " + std::to_string(pr) + " is on body " + std::to_string(b) +
            ", which has no scan lane (fingers, palm); the solver cannot take it";
      return GM_E_RANGE;
    }
  }
  return GM_OK;
}

}  // namespace

namespace {
// the process-wide settle cache of gm_set_settle_cache (calibrate_reset's first_call)
std::mutex g_settle_mu;
bool g_settle_cache_on = false, g_settle_valid = false;
int g_settle_nseg = -1;
double g_settle_eq[GM_MAX_QPOS];
}  // namespace

extern "C" {

const char* gm_version(void) { return "gripper-mi355x 0.1 (gfx950, one-wave-per-env fused env-step)"; }

int gm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int gm_create(const gm_model* model, const gm_config* cfg, const gm_object* objects, int n_objects,
              int n_envs, int env_offset, int device, uint64_t seed, gm_ctx** out) {
  if (!model || !cfg || !objects || !out || n_envs <= 0 || n_objects <= 0) return GM_E_ARG;
  *out = nullptr;
  gm_ctx* c = new gm_ctx();
  c->device = device;
  c->n_envs = n_envs;
  c->env_offset = env_offset;
  c->n_objects = n_objects;
  c->model = *model;
  c->cfg = *cfg;
  std::string err;
  int rc = build_topo(c->model, c->topo, err);
  if (rc != GM_OK) { fprintf(stderr, "gm_create: %s\n", err.c_str()); delete c; return rc; }
  if (!nseg_supported(c->model.n_seg)) {
    fprintf(stderr, "gm_create: n_seg=%d has no compiled step kernel (GM_NSEG_LIST)\n", c->model.n_seg);
    delete c;
    return GM_E_RANGE;
  }
  {
    const int CLm = c->model.n_seg + 2;
    if (c->model.nbody != 3 * CLm + 4 || c->model.nv != 3 * CLm + 8 || c->model.nq != c->model.nv + 1) {
      fprintf(stderr, "gm_create: model sizes (nbody %d, nv %d, nq %d) do not match the canonical tree for n_seg=%d\n",
              c->model.nbody, c->model.nv, c->model.nq, c->model.n_seg);
      delete c;
      return GM_E_RANGE;
    }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) {
    fprintf(stderr, "gm_create: no HIP device %d (found %d)\n", device, ndev);
    delete c;
    return GM_E_NOEXT;
  }
  *out = c;
  HIPCHK(c, hipSetDevice(device));
  HIPCHK(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
  c->stream = c->own_stream;
  HIPCHK(c, hipEventCreate(&c->ev0));
  HIPCHK(c, hipEventCreate(&c->ev1));
  HIPCHK(c, hipEventCreateWithFlags(&c->stage_ev, hipEventDisableTiming));
  c->stage_bytes = std::max(sizeof(float) * (size_t)n_envs * GM_ACTION_CODE_COUNT, sizeof(int32_t) * (size_t)n_envs);
  HIPCHK(c, c->h_stage.alloc(c->stage_bytes));
  HIPCHK(c, c->d_state.alloc((size_t)n_envs));
  HIPCHK(c, c->d_scratch.alloc(std::max(sizeof(double) * 3 * (size_t)n_envs + (size_t)n_envs + 16,
                                        sizeof(float) * 5 * (size_t)n_envs)));
  HIPCHK(c, c->d_model.alloc(1));
  HIPCHK(c, c->d_cfg.alloc(1));
  HIPCHK(c, c->d_topo.alloc(1));
  HIPCHK(c, c->d_objs.alloc((size_t)n_objects));
  HIPCHK(c, c->d_eq.alloc(GM_MAX_QPOS));
  {
    const size_t obs_b = sizeof(float) * (size_t)n_envs * (cfg->n_obs > 0 ? cfg->n_obs : 1);
    const size_t rew_b = sizeof(float) * (size_t)n_envs;
    c->out_bytes = obs_b + rew_b + (size_t)n_envs;
    HIPCHK(c, c->d_out.alloc(c->out_bytes));
    HIPCHK(c, c->h_out.alloc(c->out_bytes));
    c->d_obs = reinterpret_cast<float*>(c->d_out.get());
    c->d_rew = reinterpret_cast<float*>(c->d_out + obs_b);
    c->d_done = reinterpret_cast<uint8_t*>(c->d_out + obs_b + rew_b);
  }
  HIPCHK(c, c->d_act.alloc((size_t)n_envs * GM_ACTION_CODE_COUNT));
  HIPCHK(c, c->d_dact.alloc((size_t)n_envs));
  HIPCHK(c, c->d_mask.alloc((size_t)n_envs));
  HIPCHK(c, c->d_eval_active.alloc((size_t)n_envs));
  HIPCHK(c, c->d_spawn.alloc((size_t)n_envs));
  HIPCHK(c, c->d_order.alloc((size_t)n_envs));
  // two halves: [0, n) the costs the current launch is ordered and scheduled by (read-only
  // during it), [n, 2n) the costs it records; gm_dispatch_order_kernel moves them over
  HIPCHK(c, c->d_cost.alloc(2 * (size_t)n_envs));
  HIPCHK(c, hipMemsetAsync(c->d_cost, 0, sizeof(uint32_t) * 2 * (size_t)n_envs, c->stream));
  {
    // chunked env-step: as many workgroups as wave slots are resident (occupancy query),
    // GM_CHUNK_SUBSTEPS substeps per preemption test (default 16; 0 selects the one-shot
    // kernel).  r05 sweep on the C3 workload (tools/rollout_probe.py): 8 / 16 / 24 / 32 give
    // 5.28 / 5.22 / 5.35 / 5.21 ms per env-step for 10-step rollouts, the per-step API the same
    // 5.74-5.76 ms at 8 and 16
    const char* ev = std::getenv("GM_CHUNK_SUBSTEPS");
    c->chunk = ev ? std::atoi(ev) : 16;
    if (const char* e2 = std::getenv("GM_CHUNK_MARGIN")) c->chunk_margin = std::atoi(e2);
    if (const char* e3 = std::getenv("GM_CHUNK_YIELDS")) c->chunk_yields = std::atoi(e3);
    if (const char* e4 = std::getenv("GM_CHUNK_CMARGIN")) c->chunk_cmargin = std::atoi(e4);
    if (const char* e6 = std::getenv("GM_CHUNK_STEAL")) c->chunk_steal = std::atoi(e6) != 0;
    if (const char* e7 = std::getenv("GM_CHUNK_PRIO")) c->chunk_prio = std::atoi(e7);
    int per_cu = 0, per_cu_duo = 0, n_cu = 0;
    switch (c->model.n_seg) {
#define X(N)                                                                                              \
  case N:                                                                                                 \
    HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, gm_step_kernel<N + 2, false>, NT, 0)); \
    HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_duo, (gm_step_kernel<N + 2, false, true>), \
                                                           2 * NT, 0));                                   \
    break;
      GM_NSEG_LIST
#undef X
      default: break;
    }
    HIPCHK(c, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    // DUO when every env gets its two waves resident at once (GM_DUO = 0 / 1 forces it off
    // / on): the helper wave then costs no env a slot
    const char* ed = std::getenv("GM_DUO");
    c->duo = ed ? std::atoi(ed) != 0 : (per_cu_duo > 0 && n_envs <= per_cu_duo * n_cu);
    c->chunk_grid = std::min(n_envs, (c->duo ? per_cu_duo : per_cu) * n_cu);
    // GM_CHUNK_GRID caps the persistent grid (tests: a small batch on fewer workgroups than
    // envs, so the work queue hands envs off between waves)
    if (const char* e5 = std::getenv("GM_CHUNK_GRID")) c->chunk_grid = std::max(1, std::min(c->chunk_grid, std::atoi(e5)));
    c->chunk_cap = n_envs + c->chunk_grid;
    HIPCHK(c, c->d_chunk_ctr.alloc(GM_CQ_ALLOC));
    HIPCHK(c, hipMemsetAsync(c->d_chunk_ctr, 0, sizeof(uint32_t) * GM_CQ_ALLOC, c->stream));
    // [0, 16) launch stats, then per workgroup its end of work, then per env its start and finish
    const size_t st_words = 16 + (size_t)c->chunk_grid + 2 * (size_t)n_envs;
    HIPCHK(c, c->d_chunk_st.alloc(st_words));
    HIPCHK(c, hipMemsetAsync(c->d_chunk_st, 0, sizeof(unsigned long long) * st_words, c->stream));
    HIPCHK(c, c->d_chunk_ring.alloc(8 * GM_CQ_NB * (size_t)c->chunk_cap));
    HIPCHK(c, c->d_chunk_carry.alloc((size_t)n_envs));
    HIPCHK(c, hipMemsetAsync(c->d_chunk_ring, 0, sizeof(uint64_t) * 8 * GM_CQ_NB * (size_t)c->chunk_cap, c->stream));
  }
  hipLaunchKernelGGL(gm_dispatch_order_kernel, dim3(1), dim3(1024), 0, c->stream, c->d_cost, c->d_order, n_envs,
                     c->d_chunk_ctr, c->d_chunk_st);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemsetAsync(c->d_state, 0, sizeof(GmEnvState) * (size_t)n_envs, c->stream));
  HIPCHK(c, hipMemsetAsync(c->d_obs, 0, sizeof(float) * (size_t)n_envs * (cfg->n_obs > 0 ? cfg->n_obs : 1), c->stream));
  HIPCHK(c, hipMemsetAsync(c->d_rew, 0, sizeof(float) * (size_t)n_envs, c->stream));
  HIPCHK(c, hipMemsetAsync(c->d_done, 0, (size_t)n_envs, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_model, &c->model, sizeof(gm_model), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_cfg, &c->cfg, sizeof(gm_config), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_topo, &c->topo, sizeof(GmTopo), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_objs, objects, sizeof(gm_object) * (size_t)n_objects, hipMemcpyHostToDevice, c->stream));
  // one-time calibrate_reset settle (myfunctions.cpp:1470-1505) on env 0 -- per context, or,
  // with gm_set_settle_cache(1), once per process as the reference's function-static
  // first_call does (myfunctions.cpp:1447): later contexts with the same joint count reuse
  // the cached settle's equilibrium whatever else changed; a context whose joint count
  // differs settles again and replaces the cache (the reference's changed-joint-count
  // check sets first_call = true and keeps the new settle, myfunctions.cpp:1453-1468)
  bool from_cache = false;
  {
    std::lock_guard<std::mutex> lk(g_settle_mu);
    if (g_settle_cache_on && g_settle_valid && g_settle_nseg == c->model.n_seg) {
      HIPCHK(c, hipMemcpyAsync(c->d_eq, g_settle_eq, sizeof(double) * GM_MAX_QPOS, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      from_cache = true;
    }
  }
  if (!from_cache) {
    hipLaunchKernelGGL(gm_settle_init_kernel, dim3(1), dim3(1), 0, c->stream, c->d_state, c->d_model, c->d_topo, c->d_objs);
    DebugOut dbg{nullptr, nullptr, nullptr, nullptr, nullptr};
    HIPCHK(c, launch_step(c, 1, 1, 1, dbg));
    HIPCHK(c, hipMemcpyAsync(c->d_eq, reinterpret_cast<char*>(c->d_state.get()) + offsetof(GmEnvHot, qpos), sizeof(double) * GM_MAX_QPOS, hipMemcpyDeviceToDevice, c->stream));
    std::lock_guard<std::mutex> lk(g_settle_mu);
    if (g_settle_cache_on && (!g_settle_valid || g_settle_nseg != c->model.n_seg)) {
      HIPCHK(c, hipMemcpyAsync(g_settle_eq, c->d_eq, sizeof(double) * GM_MAX_QPOS, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      g_settle_valid = true;
      g_settle_nseg = c->model.n_seg;
    }
  }
  int threads = 256, blocks = (n_envs + threads - 1) / threads;
  hipLaunchKernelGGL(gm_init_envs_kernel, dim3(blocks), dim3(threads), 0, c->stream, c->d_state, cfg->s.random_seed,
                     (long long)env_offset, n_envs, c->model.timestep);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GM_OK;
}

void gm_destroy(gm_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  // the events and the stream after the last synchronise, by hand; the buffers with the struct
  if (c->stage_ev) (void)hipEventDestroy(c->stage_ev);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
}

const char* gm_last_error(const gm_ctx* c) { return c ? c->err.c_str() : "null context"; }
int gm_n_envs(const gm_ctx* c) { return c ? c->n_envs : 0; }
int gm_n_obs(const gm_ctx* c) { return c ? c->cfg.n_obs : 0; }
int gm_n_actions(const gm_ctx* c) { return c ? c->cfg.n_actions : 0; }

int gm_update_config(gm_ctx* c, const gm_config* cfg) {
  if (!c || !cfg) return GM_E_ARG;
  if (cfg->n_obs != c->cfg.n_obs) return fail(c, GM_E_STATE, "n_obs changed: recreate the context");
  c->cfg = *cfg;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(c->d_cfg, &c->cfg, sizeof(gm_config), hipMemcpyHostToDevice, c->stream));
  return GM_OK;
}

int gm_reset(gm_ctx* c, const uint8_t* mask, const gm_spawn* spawn) {
  if (!c) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const uint8_t* dm;
  HIPCHK(c, upload_mask(c, mask, dm));
  if (spawn)
    HIPCHK(c, hipMemcpyAsync(c->d_spawn, spawn, sizeof(gm_spawn) * (size_t)c->n_envs, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, launch_reset(c, dm, spawn ? c->d_spawn.get() : nullptr));
  if (mask || spawn) HIPCHK(c, hipStreamSynchronize(c->stream));   // host buffers may be reused
  return GM_OK;
}

int gm_spawn_object(gm_ctx* c, const uint8_t* mask, const gm_spawn* spawn) {
  if (!c || !spawn) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const uint8_t* dm;
  HIPCHK(c, upload_mask(c, mask, dm));
  HIPCHK(c, hipMemcpyAsync(c->d_spawn, spawn, sizeof(gm_spawn) * (size_t)c->n_envs, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, launch_per_env(c, gm_spawn_kernel, c->d_state, c->d_topo, dm, c->d_spawn, c->d_objs, c->n_objects, c->n_envs));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GM_OK;
}

int gm_set_motor_target(gm_ctx* c, const uint8_t* mask, const double* xyz, int n_xyz, uint8_t* in_limits) {
  if (!c || !xyz || (n_xyz != 1 && n_xyz != c->n_envs)) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)c->n_envs;
  const uint8_t* dm;
  HIPCHK(c, upload_mask(c, mask, dm));
  double* d_xyz = reinterpret_cast<double*>(c->d_scratch.get());
  uint8_t* d_ok = reinterpret_cast<uint8_t*>(d_xyz + 3 * n);
  HIPCHK(c, hipMemcpyAsync(d_xyz, xyz, sizeof(double) * 3 * (size_t)n_xyz, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(d_ok, 1, n, c->stream));
  HIPCHK(c, launch_per_env(c, gm_motor_target_kernel, c->d_state, dm, d_xyz, n_xyz == c->n_envs ? 1 : 0, d_ok,
                           c->n_envs));
  if (in_limits) HIPCHK(c, hipMemcpyAsync(in_limits, d_ok, n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // xyz / in_limits: host arrays
  return GM_OK;
}

int gm_get_sensor_si(gm_ctx* c, float* out) {
  if (!c || !out) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  float* d_out = reinterpret_cast<float*>(c->d_scratch.get());
  HIPCHK(c, launch_per_env(c, gm_sensor_si_kernel, c->d_state, d_out, c->n_envs));
  return read_back(c, out, d_out, sizeof(float) * 5 * (size_t)c->n_envs);
}

int gm_set_action(gm_ctx* c, const float* actions, int on_device) {
  if (!c || !actions) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const float* da = actions;
  if (!on_device) {
    const int rc = stage_upload(c, c->d_act, actions, sizeof(float) * (size_t)c->n_envs * c->cfg.n_actions);
    if (rc != GM_OK) return rc;
    da = c->d_act;
  }
  HIPCHK(c, launch_per_env(c, gm_action_kernel, c->d_state, c->d_model, c->d_cfg, da, nullptr, c->n_envs));
  return GM_OK;
}

int gm_set_discrete_action(gm_ctx* c, const int32_t* actions, int on_device) {
  if (!c || !actions) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const int32_t* da = actions;
  if (!on_device) {
    const int rc = stage_upload(c, c->d_dact, actions, sizeof(int32_t) * (size_t)c->n_envs);
    if (rc != GM_OK) return rc;
    da = c->d_dact;
  }
  HIPCHK(c, launch_per_env(c, gm_action_kernel, c->d_state, c->d_model, c->d_cfg, nullptr, da, c->n_envs));
  return GM_OK;
}

static bool spawn_grid_ok(const gm_spawn_params& p) {
  if (!(p.xy_increment > 0) || !(p.rot_increment > 0) || p.xrange < 0 || p.yrange < 0 || p.rotrange < 0) return false;
  const double nx = ((2 * p.xrange) / p.xy_increment) + 1, ny = ((2 * p.yrange) / p.xy_increment) + 1;
  const double nr = ((2 * p.rotrange) / p.rot_increment) + 1;
  return nx * ny < GM_SPAWN_MAX_XY + 1 && (int)nx * (int)ny <= GM_SPAWN_MAX_XY && nr < GM_SPAWN_MAX_ROT + 1;
}

int gm_spawn_into_scene(gm_ctx* c, const uint8_t* mask, const gm_spawn_params* params, int n_params, uint8_t* ok) {
  if (!c || !params || (n_params != 1 && n_params != c->n_envs)) return fail(c, GM_E_ARG, "gm_spawn_into_scene: params must hold 1 or n_envs entries");
  for (int i = 0; i < n_params; i++)
    if (!spawn_grid_ok(params[i]))
      return fail(c, GM_E_ARG, "gm_spawn_into_scene: spawn grid empty or larger than GM_SPAWN_MAX_XY / GM_SPAWN_MAX_ROT");
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf<gm_spawn_params> dp;   // (released on return: after the synchronise below, or on an error)
  DevBuf<uint8_t> dok;
  HIPCHK(c, dp.alloc((size_t)n_params));
  HIPCHK(c, dok.alloc((size_t)c->n_envs));
  HIPCHK(c, hipMemcpyAsync(dp, params, sizeof(gm_spawn_params) * (size_t)n_params, hipMemcpyHostToDevice, c->stream));
  const uint8_t* dm;
  HIPCHK(c, upload_mask(c, mask, dm));
  HIPCHK(c, launch_per_env(c, gm_spawn_into_scene_kernel, c->d_state, c->d_model, c->d_topo, c->d_objs, c->n_objects, dm,
                           dp, n_params, dok, c->n_envs));
  if (ok) HIPCHK(c, hipMemcpyAsync(ok, dok, (size_t)c->n_envs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GM_OK;
}

int gm_set_scene_spawn(gm_ctx* c, const gm_spawn_params* params, int max_tries) {
  if (!c) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (!params) { c->scene_tries = 0; HIPCHK(c, hipStreamSynchronize(c->stream)); c->d_scene.reset(); return GM_OK; }
  if (max_tries < 1 || !spawn_grid_ok(*params)) return fail(c, GM_E_ARG, "gm_set_scene_spawn: max_tries < 1 or bad spawn grid");
  if (!c->d_scene) HIPCHK(c, c->d_scene.alloc(1));
  HIPCHK(c, hipMemcpyAsync(c->d_scene, params, sizeof(gm_spawn_params), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->scene_tries = max_tries;
  return GM_OK;
}

// the driver's action fractions for every env's current state (gm_driver_action_kernel, mode: a
// GmDriver) into the caller's device array, or through d_act into its host array
static int driver_actions_out(gm_ctx* c, int mode, uint64_t seed, float jitter, float* out, int on_device) {
  HIPCHK(c, hipSetDevice(c->device));
  float* d = on_device ? out : c->d_act.get();
  HIPCHK(c, launch_per_env(c, gm_driver_action_kernel, c->d_state, c->d_model, c->d_cfg, d, c->n_envs, seed,
                           (long long)c->env_offset, jitter, mode));
  return on_device ? (int)GM_OK : read_back(c, out, d, sizeof(float) * (size_t)c->n_envs * c->cfg.n_actions);
}

int gm_scripted_actions(gm_ctx* c, uint64_t seed, float jitter, float* out, int on_device) {
  if (!c || !out) return GM_E_ARG;
  return driver_actions_out(c, GM_DRV_SCRIPT, seed, jitter, out, on_device);
}

int gm_program_actions(gm_ctx* c, uint64_t seed, float jitter, int mode, float* out, int on_device) {
  if (!c || !out || (mode != GM_DRV_PROGRAM && mode != GM_DRV_MIX)) return GM_E_ARG;
  return driver_actions_out(c, mode, seed, jitter, out, on_device);
}

int gm_random_actions(gm_ctx* c, uint64_t seed, float* out, int on_device) {
  if (!c || !out) return GM_E_ARG;
  return driver_actions_out(c, GM_DRV_RANDOM, seed, 0.0f, out, on_device);
}

int gm_rollout(gm_ctx* c, int n_steps, const gm_rollout_params* p, gm_episode_end* records) {
  if (!c || !p || n_steps < 1 ||
      (p->action_mode != GM_DRV_SCRIPT && p->action_mode != GM_DRV_RANDOM && p->action_mode != GM_DRV_PROGRAM &&
       p->action_mode != GM_DRV_MIX))
    return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (chunk_queue_on(c)) {
    const GmRolloutJob job = rollout_job(c, n_steps, (GmDriver)p->action_mode, p->seed, p->jitter,
                                         p->max_episode_steps, records);
    return timed_launch(c, &job);
  }
  return per_step_rollout(
      c, n_steps, p->max_episode_steps, records,
      [&](int) {
        const int rc = driver_actions_out(c, p->action_mode, p->seed, p->jitter, c->d_act, 1);
        return rc == GM_OK ? gm_set_action(c, c->d_act, 1) : rc;
      },
      [](int) { return (int)GM_OK; });
}

int gm_eval_record(gm_ctx* c, int max_episode_steps, uint8_t* active_inout, const gm_eval_out* out) {
  if (!c) return GM_E_ARG;
  const int rc = eval_check(c, "gm_eval_record", max_episode_steps, out);
  if (rc != GM_OK) return rc;
  if (!active_inout) return fail(c, GM_E_ARG, "gm_eval_record: no active bytes");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, launch_eval_record(c, max_episode_steps, active_inout, out, 0));
  return GM_OK;
}

int gm_evaluate(gm_ctx* c, const gm_rollout_params* p, const uint8_t* active, const gm_eval_out* out) {
  if (!c) return GM_E_ARG;
  if (!p || (p->action_mode != GM_DRV_SCRIPT && p->action_mode != GM_DRV_RANDOM && p->action_mode != GM_DRV_PROGRAM &&
             p->action_mode != GM_DRV_MIX))
    return fail(c, GM_E_ARG, "gm_evaluate: no parameters, or an action_mode other than 0, 1, 3 or 4");
  const int rc = eval_check(c, "gm_evaluate", p->max_episode_steps, out);
  if (rc != GM_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (chunk_queue_on(c))
    return eval_launch(c, rollout_job(c, p->max_episode_steps, (GmDriver)p->action_mode, p->seed, p->jitter,
                                      p->max_episode_steps, nullptr), active, out);
  return per_step_evaluate(c, p->max_episode_steps, active, out, [&](int) {
    const int r = driver_actions_out(c, p->action_mode, p->seed, p->jitter, c->d_act, 1);
    return r == GM_OK ? gm_set_action(c, c->d_act, 1) : r;
  });
}

int gm_set_random_spawn(gm_ctx* c, int enable, uint64_t seed, int position_noise_mm, int rotation_noise_deg) {
  if (!c) return GM_E_ARG;
  if (position_noise_mm < 0 || rotation_noise_deg < 0) return fail(c, GM_E_ARG, "gm_set_random_spawn: negative noise");
  c->spawn_rand.enable = enable ? 1 : 0;
  c->spawn_rand.seed = seed;
  c->spawn_rand.position_noise_mm = position_noise_mm;
  c->spawn_rand.rotation_noise_deg = rotation_noise_deg;
  c->spawn_rand.env_offset = c->env_offset;
  return GM_OK;
}

void gm_set_settle_cache(int on) {
  std::lock_guard<std::mutex> lk(g_settle_mu);
  g_settle_cache_on = on != 0;
  g_settle_valid = false;        // first_call = true: the next context settles and is kept
}

// ---------------------------------------------------------------- calibration
namespace {
uint32_t fbits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }

// calc_yield_point_load (myfunctions.cpp:3587-3595), float where the reference is float
float yield_point_load(const gm_model& m) {
  const double I = (m.finger_width * std::pow(m.finger_thickness, 3)) / 12.0;
  const float M_max = (m.yield_stress * I) / (0.5 * m.finger_thickness);
  const float F_max = M_max / m.finger_length;
  return F_max;
}

// (a base class: destroyed after CalCtx's members, so the four buffers go before their context)
struct CalOwnCtx {
  gm_ctx* c = nullptr;
  ~CalOwnCtx() { gm_destroy(c); }
};
struct CalCtx : CalOwnCtx {
  int nb = 0;
  DevBuf<double> d_dt;
  DevBuf<int32_t> d_steps;
  DevBuf<uint8_t> d_bad;
  DevBuf<float> d_gauge;
  std::vector<gm_spawn> spawn;
  // reset the first n envs (object 0 at the origin, as MjClass::reset leaves the scene),
  // give env i timestep dt[i], steps[i] substeps and the tip load, run them, read BADQACC
  int run(const std::vector<double>& dt, const std::vector<int32_t>& steps, double tip, std::vector<uint8_t>& bad,
          bool reset = true, int32_t* ran0 = nullptr) {
    const int n = (int)dt.size();
    if (n == 0) return GM_OK;
    if (reset) {
      std::vector<uint8_t> mask(nb, 0);
      for (int i = 0; i < n; i++) mask[i] = 1;
      int rc = gm_reset(c, mask.data(), spawn.data());
      if (rc != GM_OK) return rc;
    }
    HIPCHK(c, hipMemcpyAsync(d_dt, dt.data(), sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_steps, steps.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, gm_cal_launch_setup(c->stream, c->d_state, d_dt, d_steps, tip, n));
    HIPCHK(c, gm_cal_launch_step(c->model.n_seg, n, c->stream, c->d_state, c->d_model, c->d_cfg, c->d_topo));
    HIPCHK(c, gm_cal_launch_read(c->stream, c->d_state, d_bad, n));
    bad.assign(n, 0);
    HIPCHK(c, hipMemcpyAsync(bad.data(), d_bad, n, hipMemcpyDeviceToHost, c->stream));
    if (ran0)   // substeps env 0 made (GmEnvState::cal_steps after the run)
      HIPCHK(c, hipMemcpyAsync(ran0, reinterpret_cast<char*>(c->d_state.get()) + offsetof(GmEnvHot, cal_steps), sizeof(int32_t),
                               hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GM_OK;
  }
};
}  // namespace

int gm_calibrate(const gm_model* model, const gm_config* cfg, const gm_object* objects, int n_objects, int device,
                 int what, gm_calibration* out, double* trace_dt, uint8_t* trace_unstable, int max_trace) {
  if (!model || !cfg || !objects || !out || n_objects <= 0) return GM_E_ARG;
  std::memset(out, 0, sizeof(*out));
  gm_config cc = *cfg;
  cc.s.base_position_noise = 0;          // calibration runs from the same reset pose
  CalCtx k;
  k.nb = 64;
  int rc = gm_create(model, &cc, objects, n_objects, k.nb, 0, device, 0, &k.c);
  if (rc != GM_OK) return rc;
  gm_ctx* c = k.c;
  HIPCHK(c, k.d_dt.alloc(k.nb));
  HIPCHK(c, k.d_steps.alloc(k.nb));
  HIPCHK(c, k.d_bad.alloc(k.nb));
  HIPCHK(c, k.d_gauge.alloc(1));
  k.spawn.assign(k.nb, gm_spawn{0, 0.0, 0.0, 0.0});

  double timestep = model->timestep;
  if (what & GM_CAL_TIMESTEP) {
    // find_highest_stable_timestep (mjclass.cpp:4745-4854) replayed over batched results:
    // unknown candidates along the predicted path (coarse: stable, fine: unstable) are
    // simulated together, one env each, then the reference's sequence is replayed
    const float coarse_increment = 0.5e-3f, fine_increment = 50e-6f, start_value = 1.0e-3f;
    const float test_time = 1.0f, max_allowable_timestep = 20.0e-3f, tune_param = 1.0f;
    std::map<uint32_t, uint8_t> memo;
    std::vector<std::pair<float, uint8_t>> trace;
    float found = 0;
    for (int round = 0; round < 1000; round++) {
      std::vector<float> unknown;
      trace.clear();
      float next = start_value;
      bool coarse_pass = true;
      int status = 1;   // 0 done, -1 no stable timestep, 1 need evaluations
      for (int guard = 0; guard < 100000; guard++) {
        uint8_t unstable;
        auto it = memo.find(fbits(next));
        if (it != memo.end()) unstable = it->second;
        else {
          unknown.push_back(next);
          if ((int)unknown.size() >= k.nb) break;
          unstable = coarse_pass ? 0 : 1;
        }
        trace.push_back({next, unstable});
        if (unstable) { if (coarse_pass) coarse_pass = false; next -= fine_increment; }
        else { if (coarse_pass) next += coarse_increment; else { status = 0; found = next; break; } }
        if (next < fine_increment) { status = -1; break; }
        if (next > max_allowable_timestep) { next = max_allowable_timestep; coarse_pass = false; }
      }
      if (unknown.empty()) {
        if (status == -1) {
          fprintf(stderr, "gm_calibrate: no stable timestep found for the simulation\n");
          return GM_E_RANGE;
        }
        if (status == 0) break;
      }
      std::vector<double> dts(unknown.size());
      std::vector<int32_t> steps(unknown.size());
      for (size_t i = 0; i < unknown.size(); i++) {
        dts[i] = unknown[i];
        steps[i] = (int32_t)((test_time / unknown[i]) + 1);
      }
      std::vector<uint8_t> bad;
      rc = k.run(dts, steps, 0.0, bad);
      if (rc != GM_OK) return rc;
      for (size_t i = 0; i < unknown.size(); i++) memo[fbits(unknown[i])] = bad[i];
    }
    float factor;
    if (found <= 3.0e-3) factor = tune_param * 0.8;
    else if (found < 5.0e-3) factor = tune_param * 0.75;
    else if (found < 10.0e-3) factor = tune_param * 0.65;
    else factor = tune_param * 0.65;
    float final_timestep = found * factor;
    final_timestep = (float)((int)(final_timestep * 1e6) * 1e-6);
    out->search_timestep = found;
    out->n_tested = (int32_t)trace.size();
    for (int i = 0; i < (int)trace.size() && i < max_trace; i++) {
      if (trace_dt) trace_dt[i] = trace[i].first;
      if (trace_unstable) trace_unstable[i] = trace[i].second;
    }
    timestep = final_timestep;
  }
  out->timestep = timestep;
  if (what & GM_CAL_GAUGES) {
    // calibrate_simulated_sensors (mjclass.cpp:4643-4676): 0.3 s settle (wrist Z offset
    // from userdata[2], never written: 0), then validate_curve_under_force
    // (mjclass.cpp:4023-4105) with the saturation tip load for 50 s, 0.8x timestep retries
    const float yield = yield_point_load(*model);
    const float bend_gauge_normalise = cc.s.saturation_yield_factor * yield;
    double tsd = timestep;                 // s_.mujoco_timestep (double in simsettings.h:29)
    const float settle_time = 0.3f;
    std::vector<uint8_t> bad;
    rc = k.run({tsd}, {(int32_t)(settle_time / tsd)}, 0.0, bad);
    if (rc != GM_OK) return rc;
    const float time_to_settle = 50;
    const int steps_to_make = (int)(time_to_settle / tsd);
    int repeats_done = 1;
    bool first = true;
    const bool ref_retry = (what & GM_CAL_REFERENCE_RETRY) != 0;
    int left = steps_to_make;            // the reference's loop index resumes after a retry
    double tip = (double)bend_gauge_normalise;
    while (true) {
      int32_t ran = 0;
      rc = k.run({tsd}, {ref_retry ? left : steps_to_make}, tip, bad, !first, &ran);
      if (rc != GM_OK) return rc;
      first = false;
      if (bad[0]) {
        tsd *= 0.8;
        repeats_done += 1;
        if (repeats_done > 5) {
          fprintf(stderr, "gm_calibrate: curve validation unstable\n");
          return GM_E_RANGE;
        }
        if (ref_retry) {
          // reset() wiped the segment forces; `continue` resumes the step loop after the
          // unstable step, at the new timestep, unloaded
          tip = 0.0;
          left -= ran;
          if (left <= 0) {   // the unstable step was the last: only the reset remains
            rc = k.run({tsd}, {0}, 0.0, bad, true);
            if (rc != GM_OK) return rc;
            break;
          }
        }
        continue;
      }
      break;
    }
    HIPCHK(c, gm_cal_launch_gauge(c->model.n_seg, c->stream, c->d_state, c->d_model, c->d_topo, 0, k.d_gauge));
    float normalise = 0;
    HIPCHK(c, hipMemcpyAsync(&normalise, k.d_gauge, sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out->yield_load = yield;
    out->bend_gauge_normalise = bend_gauge_normalise;
    out->bending_normalise = normalise;
    out->sim_gauge_raw_to_N_factor = bend_gauge_normalise / normalise;
    out->wrist_Z_offset = 0.0f;
    out->gauge_retries = repeats_done - 1;
    out->timestep = tsd;
  }
  out->sim_steps_per_action = (int32_t)std::ceil(cc.s.time_for_action / out->timestep);
  return GM_OK;
}

int gm_step(gm_ctx* c) {
  if (!c) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  return timed_launch(c, nullptr);
}

// the last launch's queue counters (gm_chunkq.h GmCqCounter) and, with times, its time slots
static int read_chunk_counters(gm_ctx* c, uint32_t (&w)[GM_CQC_N], uint64_t* times = nullptr) {
  HIPCHK(c, hipSetDevice(c->device));
  if (times)
    HIPCHK(c, hipMemcpyAsync(times, c->d_chunk_st + GM_CQT_LAST, sizeof(uint64_t) * GM_CQT_N, hipMemcpyDeviceToHost,
                             c->stream));
  return read_back(c, w, c->d_chunk_ctr + GM_CQ_LAST, sizeof(w));
}

int gm_chunk_claim_waits(gm_ctx* c, uint32_t* out2) {
  if (!c || !out2) return GM_E_ARG;
  uint32_t w[GM_CQC_N];
  const int rc = read_chunk_counters(c, w);
  if (rc != GM_OK) return rc;
  out2[0] = w[GM_CQC_CLAIM_WAITS]; out2[1] = w[GM_CQC_CLAIM_POLLS];
  return GM_OK;
}

int gm_chunk_job_stats(gm_ctx* c, uint32_t* clk, int32_t* yields) {
  if (!c || (!clk && !yields)) return GM_E_ARG;
  if (!c->d_chunk_carry) return GM_E_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<GmChunkCarry> h((size_t)c->n_envs);
  const int rc = read_back(c, h.data(), c->d_chunk_carry, sizeof(GmChunkCarry) * h.size());
  if (rc != GM_OK) return rc;
  for (int e = 0; e < c->n_envs; e++) {
    if (clk) clk[e] = h[(size_t)e].clk;
    if (yields) yields[e] = h[(size_t)e].job_yields;
  }
  return GM_OK;
}

int gm_chunk_stats(gm_ctx* c, uint32_t* out, uint64_t* times) {
  if (!c || !out) return GM_E_ARG;
  uint32_t w[GM_CQC_N];
  const int rc = read_chunk_counters(c, w, times);
  if (rc != GM_OK) return rc;
  out[0] = std::min<uint32_t>(w[GM_CQC_FRESH], (uint32_t)c->n_envs);
  out[1] = w[GM_CQC_DONE]; out[2] = w[GM_CQC_YIELDS]; out[3] = w[GM_CQC_RESUMES];
  out[4] = (uint32_t)c->chunk; out[5] = (uint32_t)c->chunk_grid;
  out[6] = w[GM_CQC_STEALS];
  return GM_OK;
}

int gm_chunk_timeline(gm_ctx* c, uint64_t* out, int max_out) {
  if (!c || !out || max_out < 0) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const int n = std::min(max_out, c->chunk_grid + 2 * c->n_envs);
  const int rc = read_back(c, out, c->d_chunk_st + GM_CQT_TIMELINE, sizeof(uint64_t) * (size_t)n);
  return rc == GM_OK ? n : rc;
}

int gm_dispatch_info(const gm_ctx* c, int32_t* out) {
  if (!c || !out) return GM_E_ARG;
  out[0] = c->chunk; out[1] = c->chunk_grid; out[2] = c->duo ? 2 : 1; out[3] = c->last_launch_steps;
  return GM_OK;
}

int gm_last_step_ms(gm_ctx* c, float* ms) {
  if (!c || !ms || !c->timed) return GM_E_STATE;
  HIPCHK(c, hipEventSynchronize(c->ev1));
  HIPCHK(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
  return GM_OK;
}

int gm_get_obs(gm_ctx* c, float* out, int on_device) {
  if (!c || !out) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  return read_back(c, out, c->d_obs, sizeof(float) * (size_t)c->n_envs * c->cfg.n_obs, on_device);
}

int gm_get_outputs(gm_ctx* c, float* obs, float* reward, uint8_t* done) {
  if (!c || !obs || !reward || !done) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  // one copy of the contiguous obs / reward / done block into pinned memory (one DMA, no
  // pageable staging), then the three host copies
  const int rc = read_back(c, c->h_out, c->d_out, c->out_bytes);
  if (rc != GM_OK) return rc;
  const char* h = c->h_out;
  const size_t obs_b = sizeof(float) * (size_t)c->n_envs * c->cfg.n_obs;
  const size_t off_rew = reinterpret_cast<const char*>(c->d_rew) - c->d_out.get();
  const size_t off_done = reinterpret_cast<const char*>(c->d_done) - c->d_out.get();
  std::memcpy(obs, h, obs_b);
  std::memcpy(reward, h + off_rew, sizeof(float) * (size_t)c->n_envs);
  std::memcpy(done, h + off_done, (size_t)c->n_envs);
  return GM_OK;
}

int gm_get_reward_done(gm_ctx* c, float* reward, uint8_t* done, int on_device) {
  if (!c) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (reward) HIPCHK(c, hipMemcpyAsync(reward, c->d_rew, sizeof(float) * (size_t)c->n_envs, k, c->stream));
  if (done) HIPCHK(c, hipMemcpyAsync(done, c->d_done, (size_t)c->n_envs, k, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GM_OK;
}

// every env's state record into the host array out
static int fetch_states_to(gm_ctx* c, void* out) {
  HIPCHK(c, hipSetDevice(c->device));
  return read_back(c, out, c->d_state, sizeof(GmEnvState) * (size_t)c->n_envs);
}
static int fetch_states(gm_ctx* c, std::vector<GmEnvState>& h) {
  h.resize(c->n_envs);
  return fetch_states_to(c, h.data());
}

int gm_get_event_rows(gm_ctx* c, int32_t* rows, int32_t* absc, float* lastv) {
  if (!c) return GM_E_ARG;
  std::vector<GmEnvState> h;
  int rc = fetch_states(c, h);
  if (rc) return rc;
  const int W = GM_N_BINARY + GM_N_LINEAR;
  for (int e = 0; e < c->n_envs; e++) {
    for (int k = 0; k < GM_N_BINARY; k++) {
      if (rows) rows[e * W + k] = h[e].bev_row[k];
      if (absc) absc[e * W + k] = h[e].bev_abs[k];
      if (lastv) lastv[e * W + k] = (float)h[e].bev_last[k];
    }
    for (int k = 0; k < GM_N_LINEAR; k++) {
      if (rows) rows[e * W + GM_N_BINARY + k] = h[e].lev_row[k];
      if (absc) absc[e * W + GM_N_BINARY + k] = h[e].lev_abs[k];
      if (lastv) lastv[e * W + GM_N_BINARY + k] = h[e].lev_last[k];
    }
  }
  return GM_OK;
}

int gm_get_state(gm_ctx* c, double* qpos, double* qvel, double* time) {
  if (!c) return GM_E_ARG;
  std::vector<GmEnvState> h;
  int rc = fetch_states(c, h);
  if (rc) return rc;
  for (int e = 0; e < c->n_envs; e++) {
    if (qpos) for (int i = 0; i < c->model.nq; i++) qpos[(size_t)e * c->model.nq + i] = h[e].qpos[i];
    if (qvel) for (int i = 0; i < c->model.nv; i++) qvel[(size_t)e * c->model.nv + i] = h[e].qvel[i];
    if (time) time[e] = h[e].time;
  }
  return GM_OK;
}

int gm_set_state(gm_ctx* c, const double* qpos, const double* qvel) {
  if (!c) return GM_E_ARG;
  std::vector<GmEnvState> h;
  int rc = fetch_states(c, h);
  if (rc) return rc;
  for (int e = 0; e < c->n_envs; e++) {
    if (qpos) for (int i = 0; i < c->model.nq; i++) h[e].qpos[i] = qpos[(size_t)e * c->model.nq + i];
    if (qvel) for (int i = 0; i < c->model.nv; i++) h[e].qvel[i] = qvel[(size_t)e * c->model.nv + i];
  }
  HIPCHK(c, hipMemcpyAsync(c->d_state, h.data(), sizeof(GmEnvState) * (size_t)c->n_envs, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GM_OK;
}

int64_t gm_env_state_size(void) { return (int64_t)sizeof(GmEnvState); }

int gm_get_env_states(gm_ctx* c, void* out) {
  if (!c || !out) return GM_E_ARG;
  return fetch_states_to(c, out);
}

int gm_set_env_states(gm_ctx* c, const void* in) {
  if (!c || !in) return GM_E_ARG;
  const GmEnvState* h = (const GmEnvState*)in;
  // every field the kernels use as an index or a flag (a bad ring index would address
  // outside the env's sensor windows)
  for (int e = 0; e < c->n_envs; e++) {
    const GmEnvState& r = h[e];
    bool ok = r.obj_index >= 0 && r.obj_index < c->n_objects && r.extra_substeps >= 0 && r.cal_steps >= 0 &&
              r.num_action_steps >= 0 && (r.done == 0 || r.done == 1) &&
              (r.obj_type == GM_GEOM_BOX || r.obj_type == GM_GEOM_CYLINDER || r.obj_type == GM_GEOM_SPHERE);
    for (int st = 0; st < GM_NSTREAM; st++) ok = ok && r.ring_i[st] >= -1 && r.ring_i[st] < GM_RING;
    for (int k = 0; k < GM_MAX_LOCK; k++) ok = ok && (r.lock_active[k] == 0 || r.lock_active[k] == 1);
    if (!ok) return fail(c, GM_E_ARG, "gm_set_env_states: env " + std::to_string(e) + " is not a valid state");
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(c->d_state, in, sizeof(GmEnvState) * (size_t)c->n_envs, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GM_OK;
}

int gm_get_target(gm_ctx* c, double* end_xyzth, int32_t* es, int32_t* ns, double* base_xyz) {
  if (!c) return GM_E_ARG;
  std::vector<GmEnvState> h;
  int rc = fetch_states(c, h);
  if (rc) return rc;
  for (int e = 0; e < c->n_envs; e++) {
    if (end_xyzth) { end_xyzth[4 * e] = h[e].end.x; end_xyzth[4 * e + 1] = h[e].end.y; end_xyzth[4 * e + 2] = h[e].end.z; end_xyzth[4 * e + 3] = h[e].end.th; }
    if (es) { es[3 * e] = h[e].end.sx; es[3 * e + 1] = h[e].end.sy; es[3 * e + 2] = h[e].end.sz; }
    if (ns) { ns[3 * e] = h[e].next.sx; ns[3 * e + 1] = h[e].next.sy; ns[3 * e + 2] = h[e].next.sz; }
    if (base_xyz) { base_xyz[3 * e] = h[e].base[0]; base_xyz[3 * e + 1] = h[e].base[1]; base_xyz[3 * e + 2] = h[e].base[2]; }
  }
  return GM_OK;
}

int gm_get_overflow(gm_ctx* c, int32_t* counts) {
  if (!c || !counts) return GM_E_ARG;
  std::vector<GmEnvState> h;
  int rc = fetch_states(c, h);
  if (rc) return rc;
  for (int e = 0; e < c->n_envs; e++) counts[e] = h[e].overflow;
  return GM_OK;
}

void* gm_device_obs(gm_ctx* c) { return c ? c->d_obs : nullptr; }
void* gm_device_reward(gm_ctx* c) { return c ? c->d_rew : nullptr; }
void* gm_device_done(gm_ctx* c) { return c ? c->d_done : nullptr; }
void* gm_device_actions(gm_ctx* c) { return c ? c->d_act.get() : nullptr; }
void* gm_stream(gm_ctx* c) { return c ? (void*)c->stream : nullptr; }

int gm_debug_substep(gm_ctx* c, int32_t* ncon, double* contact, double* efc_force, double* qacc, int32_t* nefc,
                     double* obj_wrench) {
  if (!c) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf<int32_t> d_ncon, d_nefc;   // (released on return: after the synchronise below, or on an error)
  DevBuf<double> d_con, d_f, d_q, d_w;
  size_t n = (size_t)c->n_envs;
  HIPCHK(c, d_ncon.alloc(n));
  HIPCHK(c, d_nefc.alloc(n));
  HIPCHK(c, d_con.alloc(n * GM_MAX_CON * 16));
  HIPCHK(c, d_f.alloc(n * GM_MAX_EFC));
  HIPCHK(c, d_q.alloc(n * GM_MAX_DOF));
  HIPCHK(c, d_w.alloc(n * 6));
  DebugOut dbg{d_ncon, d_con, d_f, d_q, nullptr, d_nefc, d_w};
  HIPCHK(c, launch_step(c, c->n_envs, c->n_envs, 2, dbg));
  if (ncon) HIPCHK(c, hipMemcpyAsync(ncon, d_ncon, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
  if (nefc) HIPCHK(c, hipMemcpyAsync(nefc, d_nefc, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
  if (contact) HIPCHK(c, hipMemcpyAsync(contact, d_con, sizeof(double) * n * GM_MAX_CON * 16, hipMemcpyDeviceToHost, c->stream));
  if (efc_force) HIPCHK(c, hipMemcpyAsync(efc_force, d_f, sizeof(double) * n * GM_MAX_EFC, hipMemcpyDeviceToHost, c->stream));
  if (qacc) HIPCHK(c, hipMemcpyAsync(qacc, d_q, sizeof(double) * n * GM_MAX_DOF, hipMemcpyDeviceToHost, c->stream));
  if (obj_wrench) HIPCHK(c, hipMemcpyAsync(obj_wrench, d_w, sizeof(double) * n * 6, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GM_OK;
}

int gm_set_stream(gm_ctx* c, void* stream) {
  if (!c) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->stream = stream ? (hipStream_t)stream : c->own_stream;
  return GM_OK;
}

int gm_autoreset(gm_ctx* c, int max_episode_steps, const gm_spawn* spawn, int spawn_on_device, float* returns) {
  return gm_autoreset_episodes(c, max_episode_steps, spawn, spawn_on_device, returns, nullptr);
}

int gm_autoreset_episodes(gm_ctx* c, int max_episode_steps, const gm_spawn* spawn, int spawn_on_device,
                          float* returns, gm_episode_end* episodes) {
  static_assert(sizeof(gm_episode_end) == 12, "episode-end record is 3 x 4 bytes");
  if (!c) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const gm_spawn* ds = spawn;
  if (spawn && !spawn_on_device) {
    HIPCHK(c, hipMemcpyAsync(c->d_spawn, spawn, sizeof(gm_spawn) * (size_t)c->n_envs, hipMemcpyHostToDevice, c->stream));
    ds = c->d_spawn;
  }
  HIPCHK(c, launch_per_env(c, gm_autoreset_mask_kernel, c->d_state, c->d_done, max_episode_steps, c->d_mask, returns,
                           episodes, c->n_envs));
  HIPCHK(c, launch_reset(c, c->d_mask, ds));
  if (spawn && !spawn_on_device) HIPCHK(c, hipStreamSynchronize(c->stream));
  return GM_OK;
}

void* gm_device_reset_mask(gm_ctx* c) { return c ? c->d_mask.get() : nullptr; }

int gm_step_profiled(gm_ctx* c, uint64_t* phase_cycles) {
  if (!c || !phase_cycles) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)c->n_envs * GM_NPHASE;
  DevBuf<unsigned long long> d_ph;   // (released on return: after read_back's synchronise, or on an error)
  HIPCHK(c, d_ph.alloc(n));
  DebugOut dbg{nullptr, nullptr, nullptr, nullptr, d_ph};
  HIPCHK(c, launch_step(c, c->n_envs, c->n_envs, 0, dbg));
  return read_back(c, phase_cycles, d_ph, sizeof(unsigned long long) * n);
}

}  // extern "C"

// ---------------------------------------------------------------- on-device DQN policy
struct gm_policy {
  gm_ctx* ctx = nullptr;
  GpNet net{};
  DevBuf<float> d_params;
  DevBuf<int32_t> d_actions;
  DevBuf<float> d_q;
  DevBuf<float> d_eps;         // gm_policy_rollout's exploration thresholds, one per env-step
  int eps_cap = 0;
  std::vector<int32_t> sizes;  // the layer widths (gm_policy_set_params repacks with them)
  int64_t total = 0;           // packed floats
  DevBuf<GrArgs> d_replay;     // gm_policy_rollout_replay's launch arguments
};

static int64_t policy_layout(const int32_t* sizes, int n_sizes, GpNet* net) { return gl_layout(sizes, n_sizes, net); }

extern "C" {

int64_t gm_policy_pack(const int32_t* sizes, int n_sizes, const float* params, float* out) {
  GpNet P;
  const int64_t total = policy_layout(sizes, n_sizes, &P);
  if (total < 0 || !out) return total;
  if (!params) return GM_E_ARG;
  std::memset(out, 0, sizeof(float) * (size_t)total);
  const float* src = params;
  for (int l = 0; l < P.n_layers; l++) {
    const int in = P.width[l], outw = P.width[l + 1], ks = P.kpad[l] / 4;
    const float* W = src;            // [outw x in] row-major (torch nn.Linear.weight)
    const float* b = src + (size_t)outw * in;
    for (int t = 0; t < P.tiles[l]; t++)
      for (int s4 = 0; s4 < ks; s4++)
        for (int lane = 0; lane < 64; lane++) {
          const int j = 16 * t + (lane & 15), k = 4 * s4 + (lane >> 4);
          out[P.woff[l] + ((int64_t)t * ks + s4) * 64 + lane] = (j < outw && k < in) ? W[(size_t)j * in + k] : 0.0f;
        }
    for (int j = 0; j < outw; j++) out[P.boff[l] + j] = b[j];
    src = b + outw;
  }
  return total;
}

int gm_policy_create(gm_ctx* c, const int32_t* sizes, int n_sizes, const float* params, gm_policy** out) {
  if (!c || !sizes || !params || !out) return GM_E_ARG;
  GpNet P;
  const int64_t total = policy_layout(sizes, n_sizes, &P);
  if (total < 0) return fail(c, GM_E_RANGE, "gm_policy_create: <= 8 layers of width 1..256 expected");
  if (P.width[0] != c->cfg.n_obs || P.width[P.n_layers] != c->cfg.n_actions)
    return fail(c, GM_E_ARG, "gm_policy_create: network must map n_obs (" + std::to_string(c->cfg.n_obs) +
                                 ") to n_actions (" + std::to_string(c->cfg.n_actions) + ")");
  if (c->cfg.s.continous_actions)
    return fail(c, GM_E_ARG, "gm_policy_create: the DQN policy needs discrete actions (continous_actions = 0)");
  std::vector<float> packed((size_t)total);
  gm_policy_pack(sizes, n_sizes, params, packed.data());
  HIPCHK(c, hipSetDevice(c->device));
  gm_policy* p = new gm_policy;
  p->ctx = c;
  p->net = P;
  p->sizes.assign(sizes, sizes + n_sizes);
  p->total = total;
  hipError_t e = p->d_params.alloc((size_t)total);
  if (e == hipSuccess) e = p->d_replay.alloc(1);
  if (e == hipSuccess) e = p->d_actions.alloc((size_t)c->n_envs);
  if (e == hipSuccess) e = p->d_q.alloc((size_t)c->n_envs * c->cfg.n_actions);
  if (e == hipSuccess)
    e = hipMemcpyAsync(p->d_params, packed.data(), sizeof(float) * (size_t)total, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    gm_policy_destroy(p);
    return fail(c, GM_E_HIP, std::string("gm_policy_create: ") + hipGetErrorString(e));
  }
  *out = p;
  return GM_OK;
}

void gm_policy_destroy(gm_policy* p) {
  if (!p) return;
  if (p->ctx) {
    (void)hipSetDevice(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);   // the stream may still read d_params / d_eps
  }
  delete p;
}

int gm_policy_act(gm_policy* p, float eps, uint64_t seed, uint64_t decision) {
  if (!p || !p->ctx) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  const int blocks = (c->n_envs + GP_TILE - 1) / GP_TILE;
  hipLaunchKernelGGL(gm_policy_kernel, dim3(blocks), dim3(64), 0, c->stream, c->d_obs, c->n_envs,
                     (long long)c->env_offset, p->d_params, p->net, eps, seed, decision, p->d_actions, p->d_q);
  HIPCHK(c, hipGetLastError());
  return gm_set_discrete_action(c, p->d_actions, 1);
}

int gm_policy_set_params(gm_policy* p, const float* params) {
  if (!p || !p->ctx || !params) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<float> packed((size_t)p->total);
  gm_policy_pack(p->sizes.data(), (int)p->sizes.size(), params, packed.data());
  return stage_upload(c, p->d_params, packed.data(), sizeof(float) * (size_t)p->total);
}

}  // extern "C"

// the device-side view of a caller's replay memory for a call of n_steps env-steps that starts
// after row0 pushed transitions; false (with the message what) for a buffer the call cannot use
static bool replay_args(gm_ctx* c, const gm_replay* r, int64_t row0, int n_steps, const char* what, GrArgs& R) {
  if (!r || r->capacity < 1 || !r->state || !r->action || !r->next_state || !r->reward || !r->end || row0 < 0) {
    fail(c, GM_E_ARG, std::string(what) + ": incomplete replay memory or negative row0");
    return false;
  }
  if ((int64_t)n_steps * c->n_envs > r->capacity) {
    fail(c, GM_E_ARG, std::string(what) + ": " + std::to_string(n_steps) + " env-steps of " + std::to_string(c->n_envs) +
                          " envs would write a row of the replay memory twice (capacity " +
                          std::to_string((long long)r->capacity) + ")");
    return false;
  }
  R = GrArgs{r->state, r->action, r->next_state, r->reward, r->end, (long long)r->capacity,
             (long long)(row0 % r->capacity), c->cfg.n_obs, 0};
  return true;
}
// a thread-per-element kernel over the envs' observations on the context's stream
template <class K, class... A>
static hipError_t launch_per_obs_element(const gm_ctx* c, long long n, K kernel, const A&... args) {
  const int threads = 256;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0, c->stream, args...);
  return hipGetLastError();
}
static int policy_push(gm_policy* p, const gm_replay* r, int64_t row0, int max_ep, bool begin) {
  if (!p || !p->ctx) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  GrArgs R;
  if (!replay_args(c, r, row0, 1, begin ? "gm_policy_push_begin" : "gm_policy_push_end", R)) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const long long n = (long long)c->n_envs * c->cfg.n_obs;
  if (begin)
    HIPCHK(c, launch_per_obs_element(c, n, gm_replay_push_begin_kernel, c->d_obs, p->d_actions, c->n_envs, R));
  else
    HIPCHK(c, launch_per_obs_element(c, n, gm_replay_push_end_kernel, c->d_obs, c->d_state, c->d_rew, c->d_done,
                                     c->n_envs, max_ep, R));
  return GM_OK;
}
// gm_policy_rollout, recording into r (from row0) when r is non-NULL
static int policy_rollout(gm_policy* p, int n_steps, const float* eps, uint64_t seed, uint64_t decision0,
                          int max_episode_steps, gm_episode_end* records, const gm_replay* r, int64_t row0) {
  if (!p || !p->ctx || !eps || n_steps < 1) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  GrArgs R{};
  if (r && !replay_args(c, r, row0, n_steps, "gm_policy_rollout_replay", R)) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (chunk_queue_on(c)) {
    if (n_steps > p->eps_cap) {
      // (the stream may still read the old buffer: wait before freeing it)
      HIPCHK(c, hipStreamSynchronize(c->stream));
      p->eps_cap = 0;
      HIPCHK(c, p->d_eps.alloc((size_t)n_steps));
      p->eps_cap = n_steps;
    }
    // eps is the caller's (pageable) array: the copy owns its bytes before the call returns
    int rc = stage_upload(c, p->d_eps, eps, sizeof(float) * (size_t)n_steps);
    if (rc == GM_OK && r) rc = stage_upload(c, p->d_replay, &R, sizeof(GrArgs));
    if (rc != GM_OK) return rc;
    GmRolloutJob job = rollout_job(c, n_steps, GM_DRV_DQN, seed, 0.0f, max_episode_steps, records);
    job.pparams = p->d_params;
    job.pnet = p->net;
    job.peps = p->d_eps;
    job.pdecision = decision0;
    job.replay = r ? p->d_replay.get() : nullptr;
    return timed_launch(c, &job);
  }
  return per_step_rollout(
      c, n_steps, max_episode_steps, records,
      [&](int k) {
        const int rc = gm_policy_act(p, eps[k], seed, decision0 + (uint64_t)k);
        return rc == GM_OK && r ? gm_policy_push_begin(p, r, row0 + (int64_t)k * c->n_envs) : rc;
      },
      [&](int k) {
        return r ? gm_policy_push_end(p, r, row0 + (int64_t)k * c->n_envs, max_episode_steps) : (int)GM_OK;
      });
}

extern "C" {

int gm_policy_rollout(gm_policy* p, int n_steps, const float* eps, uint64_t seed, uint64_t decision0,
                      int max_episode_steps, gm_episode_end* records) {
  return policy_rollout(p, n_steps, eps, seed, decision0, max_episode_steps, records, nullptr, 0);
}

int gm_policy_evaluate(gm_policy* p, uint64_t seed, uint64_t decision0, int max_episode_steps, const uint8_t* active,
                       const gm_eval_out* out) {
  if (!p || !p->ctx) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  int rc = eval_action_kind(c, "gm_policy_evaluate", false, "the DQN policy");
  if (rc == GM_OK) rc = eval_check(c, "gm_policy_evaluate", max_episode_steps, out);
  if (rc != GM_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (chunk_queue_on(c)) {
    if (max_episode_steps > p->eps_cap) {
      HIPCHK(c, hipStreamSynchronize(c->stream));   // (the stream may still read the old buffer)
      p->eps_cap = 0;
      HIPCHK(c, p->d_eps.alloc((size_t)max_episode_steps));
      p->eps_cap = max_episode_steps;
    }
    // greedy: the exploration threshold of every env-step is 0
    HIPCHK(c, hipMemsetAsync(p->d_eps, 0, sizeof(float) * (size_t)max_episode_steps, c->stream));
    GmRolloutJob job = rollout_job(c, max_episode_steps, GM_DRV_DQN, seed, 0.0f, max_episode_steps, nullptr);
    job.pparams = p->d_params;
    job.pnet = p->net;
    job.peps = p->d_eps;
    job.pdecision = decision0;
    return eval_launch(c, job, active, out);
  }
  return per_step_evaluate(c, max_episode_steps, active, out,
                           [&](int k) { return gm_policy_act(p, 0.0f, seed, decision0 + (uint64_t)k); });
}

int gm_policy_push_begin(gm_policy* p, const gm_replay* replay, int64_t row0) {
  return policy_push(p, replay, row0, 0, true);
}

int gm_policy_push_end(gm_policy* p, const gm_replay* replay, int64_t row0, int max_episode_steps) {
  return policy_push(p, replay, row0, max_episode_steps, false);
}

int gm_policy_rollout_replay(gm_policy* p, int n_steps, const float* eps, uint64_t seed, uint64_t decision0,
                             int max_episode_steps, gm_episode_end* records, const gm_replay* replay, int64_t row0) {
  if (p && p->ctx && !replay) return fail(p->ctx, GM_E_ARG, "gm_policy_rollout_replay: no replay memory");
  return policy_rollout(p, n_steps, eps, seed, decision0, max_episode_steps, records, replay, row0);
}

int gm_replay_indices(int64_t size, int batch, uint64_t seed, uint64_t draw, int32_t* out) {
  if (size < 1 || size > 0x7FFFFFFFll || batch < 0 || batch > size || !out) return GM_E_ARG;
  const uint64_t key = gr_key(seed, draw);
  for (int i = 0; i < batch; i++) out[i] = (int32_t)gr_index((uint64_t)size, key, (uint64_t)i);
  return GM_OK;
}

int gm_replay_sample(gm_ctx* c, const gm_replay* replay, int64_t size, int batch, uint64_t seed, uint64_t draw,
                     const gm_replay_batch* out) {
  if (!c) return GM_E_ARG;
  if (!replay || !replay->state || !replay->action || !replay->next_state || !replay->reward || !replay->end || !out ||
      !out->state || !out->action || !out->next_state || !out->reward || !out->end || !out->index)
    return fail(c, GM_E_ARG, "gm_replay_sample: incomplete replay memory or batch arrays");
  if (size < 1 || size > replay->capacity || size > 0x7FFFFFFFll || batch < 1 || batch > size)
    return fail(c, GM_E_ARG, "gm_replay_sample: batch " + std::to_string(batch) + " of " + std::to_string((long long)size) +
                                 " stored transitions (capacity " + std::to_string((long long)replay->capacity) +
                                 "): 1 <= batch <= size <= capacity expected");
  HIPCHK(c, hipSetDevice(c->device));
  const GrArgs R{replay->state, replay->action, replay->next_state, replay->reward, replay->end,
                 (long long)replay->capacity, 0, c->cfg.n_obs, 0};
  HIPCHK(c, launch_per_obs_element(c, (long long)batch * c->cfg.n_obs, gm_replay_sample_kernel, R, (long long)size,
                                   batch, gr_key(seed, draw), *out));
  return GM_OK;
}

int gm_policy_td_target(gm_policy* target, gm_policy* online, const gm_replay_batch* batch, int n, float gamma,
                        int mask_terminal, float* y, float* next_value) {
  if (!target || !target->ctx) return GM_E_ARG;
  gm_ctx* c = target->ctx;
  if (online && online->ctx != c) return fail(c, GM_E_ARG, "gm_policy_td_target: the two policies belong to different contexts");
  if (!batch || !batch->next_state || !batch->reward || !batch->end || !y || n < 1)
    return fail(c, GM_E_ARG, "gm_policy_td_target: incomplete batch (next_state, reward, end), no y or n < 1");
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(gm_td_target_kernel, dim3((n + GP_TILE - 1) / GP_TILE), dim3(64), 0, c->stream, batch->next_state,
                     batch->reward, batch->end, n, target->d_params, target->net,
                     online ? online->d_params.get() : nullptr, online ? online->net : target->net, gamma,
                     mask_terminal, y, next_value);
  HIPCHK(c, hipGetLastError());
  return GM_OK;
}

int gm_policy_read(gm_policy* p, int32_t* actions, float* q) {
  if (!p || !p->ctx) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  if (actions)
    HIPCHK(c, hipMemcpyAsync(actions, p->d_actions, sizeof(int32_t) * (size_t)c->n_envs, hipMemcpyDeviceToHost,
                             c->stream));
  if (q)
    HIPCHK(c, hipMemcpyAsync(q, p->d_q, sizeof(float) * (size_t)c->n_envs * c->cfg.n_actions,
                             hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GM_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- on-device DQN learner
struct gm_learner {
  gm_ctx* ctx = nullptr;
  gm_policy* online = nullptr;
  gm_dqn_opt opt{};
  GlPlan plan{};
  int64_t step = 0;             // optimiser steps taken
  int64_t flat = 0;             // parameters in gm_policy_create's flat order
  DevBuf<float> d_partials;     // [GL_MAX_TILES][total] per-tile gradients
  DevBuf<float> d_tile_loss;    // [GL_MAX_TILES]
  DevBuf<float> d_grad, d_m, d_v, d_vmax;   // [total], packed order
  DevBuf<float> d_loss;         // [1] mean loss of the held gradient
  DevBuf<float> d_spill;        // the gradient kernel's rows where they do not fit LDS
  // gm_learner_train's batch and TD target
  DevBuf<float> d_state, d_next, d_reward, d_y;
  DevBuf<int32_t> d_action, d_index;
  DevBuf<uint8_t> d_end;
};

// the optimiser's launch arguments for step t (>= 1): torch's scalars, each formed in double
static GlOpt learner_opt(const gm_dqn_opt& o, int64_t t) {
  GlOpt g{};
  g.optimiser = o.optimiser;
  g.amsgrad = o.amsgrad;
  g.omb1 = (float)(1.0 - o.beta1);
  g.beta2 = (float)o.beta2;
  g.omb2 = (float)(1.0 - o.beta2);
  g.eps = (float)o.eps;
  g.wd = (float)o.weight_decay;
  g.decay = (float)(1.0 - o.lr * o.weight_decay);
  g.clamp = (float)o.grad_clamp;
  g.step_size = (float)(o.lr / (1.0 - std::pow(o.beta1, (double)t)));
  g.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(o.beta2, (double)t));
  return g;
}
// one launch of gm_learn_step_kernel over the online net's packed elements
static hipError_t learner_launch_step(gm_learner* l, bool sum, bool step, gm_policy* target, float tau, int n,
                                      float* loss_out) {
  gm_ctx* c = l->ctx;
  GlStepArgs a{};
  a.do_sum = sum;
  a.do_step = step;
  a.do_soft = target != nullptr;
  a.n_tiles = (n + GP_TILE - 1) / GP_TILE;
  a.n = n;
  a.total = (long long)l->online->total;
  a.partials = l->d_partials;
  a.tile_loss = l->d_tile_loss;
  a.grad = l->d_grad;
  a.loss = l->d_loss;
  a.loss_out = loss_out;
  a.p = l->online->d_params;
  a.m = l->d_m;
  a.v = l->d_v;
  a.vmax = l->d_vmax;
  a.target = target ? target->d_params.get() : nullptr;
  a.tau = tau;
  a.opt = learner_opt(l->opt, std::max<int64_t>(l->step, 1));
  const int threads = 256;
  hipLaunchKernelGGL(gm_learn_step_kernel, dim3((unsigned)((a.total + threads - 1) / threads)), dim3(threads), 0,
                     c->stream, a);
  return hipGetLastError();
}
static hipError_t learner_launch_grad(gm_learner* l, const float* state, const int32_t* action, const float* y, int n) {
  gm_policy* p = l->online;
  hipLaunchKernelGGL(gm_learn_grad_kernel, dim3((n + GP_TILE - 1) / GP_TILE), dim3(64), 0, l->ctx->stream, state,
                     action, y, n, p->d_params, p->net, l->plan, (int)l->opt.loss, l->d_spill, l->d_partials,
                     (long long)p->total, l->d_tile_loss);
  return hipGetLastError();
}
// packed device array -> flat host array (out) through one copy
static int learner_unpack(gm_ctx* c, const GpNet& P, int64_t total, const float* d_packed, float* out) {
  std::vector<float> packed((size_t)total);
  const int rc = read_back(c, packed.data(), d_packed, sizeof(float) * (size_t)total);
  if (rc != GM_OK) return rc;
  gl_for_each_param(P, [&](int64_t i, int64_t k) { out[i] = packed[(size_t)k]; });
  return GM_OK;
}
static bool same_sizes(const gm_policy* a, const gm_policy* b) { return a->sizes == b->sizes && a->total == b->total; }

extern "C" {

void gm_dqn_opt_default(gm_dqn_opt* out) {
  if (!out) return;
  *out = gm_dqn_opt{GM_OPT_ADAMW, 1, GM_LOSS_SMOOTH_L1, 0, 1e-4, 0.9, 0.999, 1e-8, 0.01, 100.0};
}

int gm_learner_create(gm_policy* online, const gm_dqn_opt* opt, gm_learner** out) {
  if (!online || !online->ctx || !out) return GM_E_ARG;
  gm_ctx* c = online->ctx;
  gm_dqn_opt o;
  gm_dqn_opt_default(&o);
  if (opt) o = *opt;
  if ((o.optimiser != GM_OPT_ADAM && o.optimiser != GM_OPT_ADAMW) || (o.loss != GM_LOSS_SMOOTH_L1 && o.loss != GM_LOSS_MSE))
    return fail(c, GM_E_ARG, "gm_learner_create: optimiser must be GM_OPT_ADAM / GM_OPT_ADAMW, loss GM_LOSS_SMOOTH_L1 / GM_LOSS_MSE");
  if (!(o.lr >= 0) || !(o.beta1 >= 0 && o.beta1 < 1) || !(o.beta2 >= 0 && o.beta2 < 1) || !(o.eps >= 0) || !(o.weight_decay >= 0))
    return fail(c, GM_E_ARG, "gm_learner_create: lr, eps, weight_decay >= 0 and betas in [0, 1) expected");
  HIPCHK(c, hipSetDevice(c->device));
  gm_learner* l = new gm_learner;
  l->ctx = c;
  l->online = online;
  l->opt = o;
  l->plan = gl_plan(online->net);
  l->flat = gl_flat_count(online->net);
  const size_t total = (size_t)online->total, n_obs = (size_t)c->cfg.n_obs;
  hipError_t e = l->d_partials.alloc(total * GL_MAX_TILES);
  if (e == hipSuccess) e = l->d_tile_loss.alloc(GL_MAX_TILES);
  if (e == hipSuccess) e = l->d_grad.alloc(total);
  if (e == hipSuccess) e = l->d_m.alloc(total);
  if (e == hipSuccess) e = l->d_v.alloc(total);
  if (e == hipSuccess) e = l->d_vmax.alloc(total);
  if (e == hipSuccess) e = l->d_loss.alloc(1);
  if (e == hipSuccess) e = l->d_spill.alloc(l->plan.total > GL_ARENA ? (size_t)l->plan.total * GL_MAX_TILES : 1);
  if (e == hipSuccess) e = l->d_state.alloc(n_obs * GL_MAX_BATCH);
  if (e == hipSuccess) e = l->d_next.alloc(n_obs * GL_MAX_BATCH);
  if (e == hipSuccess) e = l->d_reward.alloc(GL_MAX_BATCH);
  if (e == hipSuccess) e = l->d_y.alloc(GL_MAX_BATCH);
  if (e == hipSuccess) e = l->d_action.alloc(GL_MAX_BATCH);
  if (e == hipSuccess) e = l->d_index.alloc(GL_MAX_BATCH);
  if (e == hipSuccess) e = l->d_end.alloc(GL_MAX_BATCH);
  for (float* z : {l->d_grad.get(), l->d_m.get(), l->d_v.get(), l->d_vmax.get()})
    if (e == hipSuccess) e = hipMemsetAsync(z, 0, sizeof(float) * total, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(l->d_loss, 0, sizeof(float), c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    gm_learner_destroy(l);
    return fail(c, GM_E_HIP, std::string("gm_learner_create: ") + hipGetErrorString(e));
  }
  *out = l;
  return GM_OK;
}

void gm_learner_destroy(gm_learner* l) {
  if (!l) return;
  if (l->ctx) {
    (void)hipSetDevice(l->ctx->device);
    (void)hipStreamSynchronize(l->ctx->stream);   // the stream may still use the learner's buffers
  }
  delete l;
}

int gm_learner_grad(gm_learner* l, const gm_replay_batch* batch, const float* y, int n) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  if (!batch || !batch->state || !batch->action || !y || n < 1)
    return fail(c, GM_E_ARG, "gm_learner_grad: incomplete batch (state, action), no y or n < 1");
  if (n > GL_MAX_BATCH)
    return fail(c, GM_E_ARG, "gm_learner_grad: " + std::to_string(n) + " rows, the learner holds " +
                                 std::to_string(GL_MAX_BATCH));
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, learner_launch_grad(l, batch->state, batch->action, y, n));
  HIPCHK(c, learner_launch_step(l, true, false, nullptr, 0.0f, n, nullptr));
  return GM_OK;
}

int gm_learner_step(gm_learner* l) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  l->step++;
  HIPCHK(c, learner_launch_step(l, false, true, nullptr, 0.0f, 1, nullptr));
  return GM_OK;
}

int gm_learner_read(gm_learner* l, float* grad_flat, float* loss) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  if (grad_flat) {
    const int rc = learner_unpack(c, l->online->net, l->online->total, l->d_grad, grad_flat);
    if (rc != GM_OK) return rc;
  }
  return loss ? read_back(c, loss, l->d_loss, sizeof(float)) : (int)GM_OK;
}

int gm_learner_get_state(gm_learner* l, int64_t* step, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  if (step) *step = l->step;
  const float* src[3] = {l->d_m, l->d_v, l->d_vmax};
  float* dst[3] = {exp_avg, exp_avg_sq, max_exp_avg_sq};
  for (int i = 0; i < 3; i++)
    if (dst[i]) {
      const int rc = learner_unpack(c, l->online->net, l->online->total, src[i], dst[i]);
      if (rc != GM_OK) return rc;
    }
  return GM_OK;
}

int gm_learner_set_state(gm_learner* l, const int64_t* step, const float* exp_avg, const float* exp_avg_sq,
                         const float* max_exp_avg_sq) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  if (step && *step < 0) return fail(c, GM_E_ARG, "gm_learner_set_state: negative step");
  HIPCHK(c, hipSetDevice(c->device));
  const float* src[3] = {exp_avg, exp_avg_sq, max_exp_avg_sq};
  float* dst[3] = {l->d_m, l->d_v, l->d_vmax};
  gm_policy* p = l->online;
  std::vector<float> packed((size_t)p->total);
  for (int i = 0; i < 3; i++)
    if (src[i]) {
      gm_policy_pack(p->sizes.data(), (int)p->sizes.size(), src[i], packed.data());
      const int rc = stage_upload(c, dst[i], packed.data(), sizeof(float) * (size_t)p->total);
      if (rc != GM_OK) return rc;
    }
  if (step) l->step = *step;
  return GM_OK;
}

int gm_policy_get_params(gm_policy* p, float* flat) {
  if (!p || !p->ctx || !flat) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  return learner_unpack(c, p->net, p->total, p->d_params, flat);
}

int gm_policy_get_packed(gm_policy* p, float* packed) {
  if (!p || !p->ctx || !packed) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  return read_back(c, packed, p->d_params, sizeof(float) * (size_t)p->total);
}

int gm_policy_soft_update(gm_policy* target, gm_policy* online, float tau) {
  if (!target || !target->ctx || !online) return GM_E_ARG;
  gm_ctx* c = target->ctx;
  if (online->ctx != c) return fail(c, GM_E_ARG, "gm_policy_soft_update: the two policies belong to different contexts");
  if (!same_sizes(target, online)) return fail(c, GM_E_ARG, "gm_policy_soft_update: the two policies differ in their layer sizes");
  if (!(tau >= 0.0f && tau <= 1.0f)) return fail(c, GM_E_ARG, "gm_policy_soft_update: tau in [0, 1] expected");
  HIPCHK(c, hipSetDevice(c->device));
  GlStepArgs a{};
  a.do_soft = 1;
  a.total = (long long)online->total;
  a.p = online->d_params;
  a.target = target->d_params;
  a.tau = tau;
  const int threads = 256;
  hipLaunchKernelGGL(gm_learn_step_kernel, dim3((unsigned)((a.total + threads - 1) / threads)), dim3(threads), 0,
                     c->stream, a);
  HIPCHK(c, hipGetLastError());
  return GM_OK;
}

int gm_learner_train(gm_learner* l, gm_policy* target, const gm_replay* replay, int64_t size, int batch, uint64_t seed,
                     uint64_t draw0, int n_updates, float gamma, int double_dqn, int mask_terminal, float tau,
                     float* losses) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  gm_policy* online = l->online;
  if (target && target->ctx != c) return fail(c, GM_E_ARG, "gm_learner_train: the two policies belong to different contexts");
  if (target && !same_sizes(target, online)) return fail(c, GM_E_ARG, "gm_learner_train: the two policies differ in their layer sizes");
  if (n_updates < 1) return fail(c, GM_E_ARG, "gm_learner_train: n_updates < 1");
  if (batch > GL_MAX_BATCH)
    return fail(c, GM_E_ARG, "gm_learner_train: batch " + std::to_string(batch) + ", the learner holds " +
                                 std::to_string(GL_MAX_BATCH));
  if (tau > 0.0f && (!target || target == online || !(tau <= 1.0f)))
    return fail(c, GM_E_ARG, "gm_learner_train: a soft update needs a target policy of its own and tau <= 1");
  const bool soft = tau > 0.0f;
  gm_policy* tdnet = target ? target : online;
  const gm_replay_batch b{l->d_state, l->d_action, l->d_next, l->d_reward, l->d_end, l->d_index};
  for (int u = 0; u < n_updates; u++) {
    int rc = gm_replay_sample(c, replay, size, batch, seed, draw0 + (uint64_t)u, &b);   // (validates replay, size, batch)
    if (rc == GM_OK) rc = gm_policy_td_target(tdnet, double_dqn ? online : nullptr, &b, batch, gamma, mask_terminal, l->d_y, nullptr);
    if (rc != GM_OK) return rc;
    HIPCHK(c, learner_launch_grad(l, l->d_state, l->d_action, l->d_y, batch));
    l->step++;
    HIPCHK(c, learner_launch_step(l, true, true, soft ? target : nullptr, tau, batch, losses ? losses + u : nullptr));
  }
  return GM_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- on-device PPO actor-critic
struct gm_ac {
  gm_ctx* ctx = nullptr;
  GaNet net{};
  int64_t total = 0;           // packed floats
  int64_t n_raw = 0;           // floats of the caller's (state_dict order) parameters
  std::vector<int32_t> asz, csz;
  DevBuf<float> d_params;
  DevBuf<GaArgs> d_args;       // gm_ac_rollout's launch arguments
  // gm_ac_evaluate's one-row scratch trajectory (made at its first call): the float rows obs,
  // act, mu, logp, val, rew, boot, last_val in one allocation, and the end bytes
  DevBuf<float> d_eval_rows;
  DevBuf<uint8_t> d_eval_end;
};

static_assert(GA_MAX_ACT >= GM_ACTION_CODE_COUNT, "the sampler's rows hold every action");

static int64_t ac_layout(const int32_t* asz, int na, const int32_t* csz, int nc, GaNet* net, int64_t* n_raw,
                         int categorical = 0) {
  return gq_layout(asz, na, csz, nc, net, n_raw, categorical);
}

// the device-side view of a caller's trajectory buffer
static void ac_fill(GaArgs& A, const gm_ac* p, const gm_ac_traj* t, int sample, float noise, uint64_t seed,
                    uint64_t decision0) {
  A.net = p->net;
  A.params = p->d_params;
  A.t_obs = t->obs; A.t_act = t->act; A.t_logp = t->logp; A.t_val = t->val; A.t_rew = t->rew; A.t_end = t->end;
  A.t_boot = t->boot; A.t_last_val = t->last_val; A.t_mu = t->mu;
  A.t_idx = nullptr;
  A.sample = sample;
  A.noise = noise;
  A.seed = seed;
  A.decision0 = decision0;
}
static bool ac_traj_ok(const gm_ac_traj* t) {
  return t && t->capacity >= 1 && t->obs && t->act && t->logp && t->val && t->rew && t->end && t->boot && t->last_val;
}
// One per-step call (what: 0 gm_ac_act, 1 gm_ac_record, 2 gm_ac_finish) on trajectory row k: the
// checks (bad: the message for a bad buffer, row or noise), the device, gm_ac_kernel
static int ac_step(gm_ac* p, const gm_ac_traj* t, int k, int what, int max_ep, const char* bad, int sample = 0,
                   float noise = 0.0f, uint64_t seed = 0, uint64_t decision0 = 0) {
  if (!p || !p->ctx) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  if (!ac_traj_ok(t) || k < 0 || k >= t->capacity || !(noise >= 0.0f)) return fail(c, GM_E_ARG, bad);
  if (p->net.categorical && noise != 0.0f)
    return fail(c, GM_E_ARG, "gm_ac_act: a categorical actor takes no exploration noise (noise must be 0)");
  HIPCHK(c, hipSetDevice(c->device));
  GaArgs A{};
  ac_fill(A, p, t, sample, noise, seed, decision0);
  if (p->net.categorical && what == 0) A.t_idx = c->d_dact;
  const int blocks = (c->n_envs + GP_TILE - 1) / GP_TILE;
  hipLaunchKernelGGL(gm_ac_kernel, dim3(blocks), dim3(64), 0, c->stream, what, c->d_obs, c->d_state, c->d_rew,
                     c->d_done, c->n_envs, (long long)c->env_offset, A, k, max_ep);
  HIPCHK(c, hipGetLastError());
  return GM_OK;
}

// gm_ac_pack (categorical 0) and gm_ac_pack_categorical (1)
static int64_t ac_pack(int categorical, const int32_t* actor_sizes, int n_actor, const int32_t* critic_sizes,
                       int n_critic, const float* params, float* out, int64_t* off2) {
  GaNet N;
  if (!actor_sizes || !critic_sizes || n_actor < 2 || n_critic < 2) return -1;
  const int64_t total = ac_layout(actor_sizes, n_actor, critic_sizes, n_critic, &N, nullptr, categorical);
  if (total < 0) return total;
  if (off2) { off2[0] = N.critic_off; off2[1] = N.log_std_off; }
  if (!out) return total;
  if (!params) return GM_E_ARG;
  const float* src = params;
  gm_policy_pack(actor_sizes, n_actor, src, out);
  for (int l = 0; l + 1 < n_actor; l++) src += (size_t)actor_sizes[l + 1] * actor_sizes[l] + actor_sizes[l + 1];
  gm_policy_pack(critic_sizes, n_critic, src, out + N.critic_off);
  for (int l = 0; l + 1 < n_critic; l++) src += (size_t)critic_sizes[l + 1] * critic_sizes[l] + critic_sizes[l + 1];
  if (!categorical) std::memcpy(out + N.log_std_off, src, sizeof(float) * (size_t)actor_sizes[n_actor - 1]);
  return total;
}

// gm_ac_create (categorical 0) and gm_ac_create_categorical (1); the messages name the caller's entry point
static int ac_create(int categorical, gm_ctx* c, const int32_t* actor_sizes, int n_actor, const int32_t* critic_sizes,
                     int n_critic, const float* params, gm_ac** out) {
  const std::string who = categorical ? "gm_ac_create_categorical: " : "gm_ac_create: ";
  if (!c || !actor_sizes || !critic_sizes || !params || !out || n_actor < 2 || n_critic < 2) return GM_E_ARG;
  GaNet N;
  int64_t n_raw = 0;
  const int64_t total = ac_layout(actor_sizes, n_actor, critic_sizes, n_critic, &N, &n_raw, categorical);
  if (total < 0) return fail(c, GM_E_ARG, who + "<= 8 layers of width 1..256 expected");
  if (!categorical && !c->cfg.s.continous_actions)
    return fail(c, GM_E_ARG, who + "the Gaussian actor needs continuous actions (continous_actions != 0)");
  if (categorical && c->cfg.s.continous_actions)
    return fail(c, GM_E_ARG, who + "the categorical actor needs discrete actions (continous_actions == 0)");
  if (N.actor.width[0] != c->cfg.n_obs || N.actor.width[N.actor.n_layers] != c->cfg.n_actions)
    return fail(c, GM_E_ARG, who + "the actor must map n_obs (" + std::to_string(c->cfg.n_obs) +
                                 ") to n_actions (" + std::to_string(c->cfg.n_actions) + ")");
  if (N.critic.width[0] != c->cfg.n_obs || N.critic.width[N.critic.n_layers] != 1)
    return fail(c, GM_E_ARG, who + "the critic must map n_obs (" + std::to_string(c->cfg.n_obs) + ") to 1");
  HIPCHK(c, hipSetDevice(c->device));
  gm_ac* p = new gm_ac;
  p->ctx = c;
  p->net = N;
  p->total = total;
  p->n_raw = n_raw;
  p->asz.assign(actor_sizes, actor_sizes + n_actor);
  p->csz.assign(critic_sizes, critic_sizes + n_critic);
  hipError_t e = p->d_params.alloc((size_t)total);
  if (e == hipSuccess) e = p->d_args.alloc(1);
  if (e != hipSuccess) {
    gm_ac_destroy(p);
    return fail(c, GM_E_HIP, who + hipGetErrorString(e));
  }
  const int rc = gm_ac_set_params(p, params);
  if (rc != GM_OK) { gm_ac_destroy(p); return rc; }
  *out = p;
  return GM_OK;
}

extern "C" {

int64_t gm_ac_pack(const int32_t* actor_sizes, int n_actor, const int32_t* critic_sizes, int n_critic,
                   const float* params, float* out, int64_t* off2) {
  return ac_pack(0, actor_sizes, n_actor, critic_sizes, n_critic, params, out, off2);
}

int64_t gm_ac_pack_categorical(const int32_t* actor_sizes, int n_actor, const int32_t* critic_sizes, int n_critic,
                               const float* params, float* out, int64_t* off2) {
  return ac_pack(1, actor_sizes, n_actor, critic_sizes, n_critic, params, out, off2);
}

int gm_ac_create(gm_ctx* c, const int32_t* actor_sizes, int n_actor, const int32_t* critic_sizes, int n_critic,
                 const float* params, gm_ac** out) {
  return ac_create(0, c, actor_sizes, n_actor, critic_sizes, n_critic, params, out);
}

int gm_ac_create_categorical(gm_ctx* c, const int32_t* actor_sizes, int n_actor, const int32_t* critic_sizes,
                             int n_critic, const float* params, gm_ac** out) {
  return ac_create(1, c, actor_sizes, n_actor, critic_sizes, n_critic, params, out);
}

void gm_ac_destroy(gm_ac* p) {
  if (!p) return;
  if (p->ctx) {
    (void)hipSetDevice(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);
  }
  delete p;
}

int gm_ac_set_params(gm_ac* p, const float* params) {
  if (!p || !p->ctx || !params) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<float> packed((size_t)p->total);
  ac_pack(p->net.categorical, p->asz.data(), (int)p->asz.size(), p->csz.data(), (int)p->csz.size(), params,
          packed.data(), nullptr);
  return stage_upload(c, p->d_params, packed.data(), sizeof(float) * (size_t)p->total);
}

int gm_ac_act(gm_ac* p, const gm_ac_traj* traj, int k, int sample, float noise, uint64_t seed, uint64_t decision) {
  // (the kernel draws with decision0 + k)
  const int rc =
      ac_step(p, traj, k, 0, 0, "gm_ac_act: incomplete trajectory buffer, k outside its capacity or negative noise",
              sample, noise, seed, decision - (uint64_t)k);
  if (rc != GM_OK) return rc;
  gm_ctx* c = p->ctx;
  // (categorical: the kernel left the chosen indices in d_dact; gm_policy_act's path, lift substeps included)
  if (p->net.categorical) return gm_set_discrete_action(c, c->d_dact, 1);
  return gm_set_action(c, traj->act + (size_t)k * c->n_envs * c->cfg.n_actions, 1);
}

int gm_ac_record(gm_ac* p, const gm_ac_traj* traj, int k, int max_episode_steps) {
  return ac_step(p, traj, k, 1, max_episode_steps, "gm_ac_record: incomplete trajectory buffer or k outside its capacity");
}

int gm_ac_finish(gm_ac* p, const gm_ac_traj* traj, int k_last) {
  return ac_step(p, traj, k_last, 2, 0, "gm_ac_finish: incomplete trajectory buffer or k_last outside its capacity");
}

int gm_ac_rollout(gm_ac* p, const gm_ac_traj* traj, int n_steps, int sample, float noise, uint64_t seed,
                  uint64_t decision0, int max_episode_steps, gm_episode_end* records) {
  if (!p || !p->ctx) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  if (!ac_traj_ok(traj) || n_steps < 1 || n_steps > traj->capacity || !(noise >= 0.0f))
    return fail(c, GM_E_ARG, "gm_ac_rollout: incomplete trajectory buffer, n_steps outside its capacity or negative noise");
  if (p->net.categorical && noise != 0.0f)
    return fail(c, GM_E_ARG, "gm_ac_rollout: a categorical actor takes no exploration noise (noise must be 0)");
  HIPCHK(c, hipSetDevice(c->device));
  if (chunk_queue_on(c)) {
    GaArgs A{};
    ac_fill(A, p, traj, sample, noise, seed, decision0);
    const int rc = stage_upload(c, p->d_args, &A, sizeof(GaArgs));
    if (rc != GM_OK) return rc;
    GmRolloutJob job = rollout_job(c, n_steps, GM_DRV_AC, seed, 0.0f, max_episode_steps, records);
    job.ac = p->d_args;
    return timed_launch(c, &job);
  }
  const int rc = per_step_rollout(
      c, n_steps, max_episode_steps, records,
      [&](int k) { return gm_ac_act(p, traj, k, sample, noise, seed, decision0 + (uint64_t)k); },
      [&](int k) { return gm_ac_record(p, traj, k, max_episode_steps); });
  return rc == GM_OK ? gm_ac_finish(p, traj, n_steps - 1) : rc;
}

int gm_ac_evaluate(gm_ac* p, int sample, uint64_t seed, uint64_t decision0, int max_episode_steps,
                   const uint8_t* active, const gm_eval_out* out) {
  if (!p || !p->ctx) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  int rc = eval_action_kind(c, "gm_ac_evaluate", !p->net.categorical,
                            p->net.categorical ? "the categorical actor" : "the Gaussian actor");
  if (rc == GM_OK) rc = eval_check(c, "gm_ac_evaluate", max_episode_steps, out);
  if (rc != GM_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)c->n_envs, n_obs = (size_t)c->cfg.n_obs, na = (size_t)c->cfg.n_actions;
  if (!p->d_eval_rows) {
    HIPCHK(c, p->d_eval_rows.alloc(n * (n_obs + 2 * na + 5)));
    HIPCHK(c, p->d_eval_end.alloc(n));
  }
  // the actor's phases write one trajectory row whatever the env-step: nothing of it is kept
  float* f = p->d_eval_rows;
  gm_ac_traj t{};
  t.capacity = 1;
  t.obs = f; f += n * n_obs;
  t.act = f; f += n * na;
  t.mu = f; f += n * na;
  t.logp = f; f += n;
  t.val = f; f += n;
  t.rew = f; f += n;
  t.boot = f; f += n;
  t.last_val = f;
  t.end = p->d_eval_end;
  if (chunk_queue_on(c)) {
    GaArgs A{};
    ac_fill(A, p, &t, sample, 0.0f, seed, decision0);
    A.one_row = 1;
    rc = stage_upload(c, p->d_args, &A, sizeof(GaArgs));
    if (rc != GM_OK) return rc;
    GmRolloutJob job = rollout_job(c, max_episode_steps, GM_DRV_AC, seed, 0.0f, max_episode_steps, nullptr);
    job.ac = p->d_args;
    return eval_launch(c, job, active, out);
  }
  return per_step_evaluate(c, max_episode_steps, active, out,
                           [&](int k) { return gm_ac_act(p, &t, 0, sample, 0.0f, seed, decision0 + (uint64_t)k); });
}

int gm_ac_gae(gm_ctx* c, const gm_ac_traj* traj, int n_steps, float gamma, float lam, float* adv, float* ret) {
  if (!c) return GM_E_ARG;
  if (!traj || !traj->rew || !traj->val || !traj->end || !traj->boot || !traj->last_val || !adv || !ret ||
      n_steps < 1 || n_steps > traj->capacity)
    return fail(c, GM_E_ARG, "gm_ac_gae: incomplete trajectory buffer or n_steps outside its capacity");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, launch_per_env(c, gm_ac_gae_kernel, traj->rew, traj->val, traj->end, traj->boot, traj->last_val, c->n_envs,
                           n_steps, gamma, lam, adv, ret));
  return GM_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- on-device PPO learner
struct gm_ppo_learner {
  gm_ctx* ctx = nullptr;
  gm_ac* ac = nullptr;
  gm_ppo_opt opt{};
  int groups = 0;
  GlPlan plan_pi{}, plan_vf{};
  int64_t step_pi = 0, step_vf = 0;         // optimiser steps taken
  DevBuf<float> d_partials;                 // [groups][total] one running gradient per workgroup
  DevBuf<float> d_wg;                       // [groups][GQ_INFO]
  DevBuf<float> d_grad, d_m, d_v, d_vmax;   // [total], packed order; policy entries pi's, critic entries vf's
  DevBuf<float> d_scalars;                  // [3][GQ_SCALARS]: the held gradient's, update's first and last
  DevBuf<int32_t> d_stop;                   // [2] the KL stop's latch, policy iterations that stepped
  DevBuf<float> d_spill;                    // [groups][spill_stride] the gradient kernels' rows where they do not fit LDS
  long long spill_stride = 1;
  DevBuf<float> d_adv, d_ret;               // gm_ppo_learner_update's advantages and returns
  size_t rows_cap = 0;
};

// the optimiser's launch arguments of step t of pi (policy) or vf, through the DQN learner's rule
static GlOpt ppo_learner_opt(const gm_ppo_opt& o, bool policy, int64_t t) {
  gm_dqn_opt d{};
  d.optimiser = o.optimiser;
  d.amsgrad = o.optimiser == GM_OPT_ADAMW;
  d.lr = policy ? o.learning_rate_pi : o.learning_rate_vf;
  d.beta1 = o.adam_beta1;
  d.beta2 = o.adam_beta2;
  d.eps = 1e-8;
  d.weight_decay = o.optimiser == GM_OPT_ADAMW ? 0.01 : 0.0;
  d.grad_clamp = o.grad_clamp_value > 0 ? o.grad_clamp_value : 0.0;
  return learner_opt(d, t);
}
// the gradient kernel of one net over a batch, then the reduce kernel; stop: d_stop inside
// gm_ppo_learner_update's policy loop, else NULL; first / last: update's info rows or NULL
static hipError_t ppo_launch_grad(gm_ppo_learner* l, bool policy, const gm_ppo_batch& b, int* stop, float* first,
                                  float* last) {
  gm_ctx* c = l->ctx;
  const gm_ac* p = l->ac;
  const GaNet& N = p->net;
  const int n_act = N.actor.width[N.actor.n_layers];
  const int n_ls = N.categorical ? 0 : n_act;     // log_std entries, behind the critic
  GqGradArgs a{};
  a.obs = b.obs; a.act = b.act; a.logp_old = b.logp; a.adv = b.adv; a.ret = b.ret;
  a.n = b.n;
  a.params = p->d_params;
  a.net = policy ? N.actor : N.critic;
  a.plan = policy ? l->plan_pi : l->plan_vf;
  a.net_off = policy ? 0 : N.critic_off;
  a.net_total = policy ? N.critic_off : N.log_std_off - N.critic_off;
  a.lds_part = gq_lds_part(a.plan, a.net_total);
  a.log_std_off = N.log_std_off;
  a.n_groups = l->groups;
  a.use_kl = l->opt.use_kl_penalty != 0;
  a.clip_lo = (float)(1.0 - l->opt.clip_ratio);
  a.clip_hi = (float)(1.0 + l->opt.clip_ratio);
  a.beta = (float)l->opt.kl_penalty_coefficient;
  a.spill = l->d_spill;
  a.spill_stride = l->spill_stride;
  a.partials = l->d_partials;
  a.total = (long long)p->total;
  a.wg_info = l->d_wg;
  a.stop = stop;
  a.use_ent = l->opt.use_entropy_regularisation != 0;
  a.c_ent = (float)l->opt.entropy_coefficient;
  const size_t lds = sizeof(float) * (size_t)(a.plan.total <= GL_ARENA ? a.plan.total + (a.lds_part ? a.net_total : 0) : 0);
  if (policy && N.categorical)
    hipLaunchKernelGGL(gm_ppo_grad_pi_cat_kernel, dim3(l->groups), dim3(64), lds, c->stream, a);
  else if (policy)
    hipLaunchKernelGGL(gm_ppo_grad_pi_kernel, dim3(l->groups), dim3(64), lds, c->stream, a);
  else
    hipLaunchKernelGGL(gm_ppo_grad_vf_kernel, dim3(l->groups), dim3(64), lds, c->stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const long long tiles = (b.n + GP_TILE - 1) / GP_TILE;
  const long long ta = N.critic_off, tc = N.log_std_off - N.critic_off;
  GqReduceArgs r{};
  r.partials = l->d_partials;
  r.total = a.total;
  r.n_parts = (int)std::min<long long>(l->groups, tiles);
  r.count = policy ? ta + n_ls : tc;
  r.first = policy ? 0 : ta;
  r.gap_at = policy ? ta : r.count;
  r.gap_len = policy ? tc : 0;
  r.grad = l->d_grad;
  r.wg_info = l->d_wg;
  r.n = b.n;
  r.policy = policy;
  r.use_kl = a.use_kl;
  r.use_ent = l->opt.use_entropy_regularisation != 0;
  r.beta = a.beta;
  r.c_ent = (float)l->opt.entropy_coefficient;
  r.params = p->d_params;
  r.log_std_off = N.log_std_off;
  r.n_act = n_act;
  r.scalars = l->d_scalars;
  r.first_out = first;
  r.last_out = last;
  r.stop = stop;
  r.kl_stop = l->opt.max_kl_ratio * l->opt.target_kl;
  r.categorical = N.categorical;
  const int threads = 256;
  hipLaunchKernelGGL(gm_ppo_reduce_kernel, dim3((unsigned)((r.count + threads - 1) / threads)), dim3(threads), 0,
                     c->stream, r);
  return hipGetLastError();
}
// gm_learn_step_kernel over one optimiser's elements, as step t; skip: the KL stop's latch or NULL
static hipError_t ppo_launch_step(gm_ppo_learner* l, bool policy, int64_t t, const int* skip) {
  gm_ctx* c = l->ctx;
  const GaNet& N = l->ac->net;
  const long long ta = N.critic_off, tc = N.log_std_off - N.critic_off;
  const long long first = policy ? 0 : ta;
  GlStepArgs a{};
  a.do_step = 1;
  a.total = policy ? ta + (N.categorical ? 0 : N.actor.width[N.actor.n_layers]) : tc;
  a.gap_at = policy ? ta : 0;
  a.gap_len = policy ? tc : 0;
  a.grad = l->d_grad + first;
  a.p = l->ac->d_params + first;
  a.m = l->d_m + first;
  a.v = l->d_v + first;
  a.vmax = l->d_vmax + first;
  a.opt = ppo_learner_opt(l->opt, policy, std::max<int64_t>(t, 1));
  a.skip = skip;
  const int threads = 256;
  hipLaunchKernelGGL(gm_learn_step_kernel, dim3((unsigned)((a.total + threads - 1) / threads)), dim3(threads), 0,
                     c->stream, a);
  return hipGetLastError();
}
static bool ppo_batch_ok(const gm_ppo_batch* b, bool policy) {
  return b && b->n >= 1 && b->obs && (policy ? (b->act && b->logp && b->adv) : b->ret != nullptr);
}
// a packed device array of the blob -> flat host array
static int ac_unpack(gm_ctx* c, const gm_ac* p, const float* d_packed, float* out) {
  std::vector<float> packed((size_t)p->total);
  const int rc = read_back(c, packed.data(), d_packed, sizeof(float) * (size_t)p->total);
  if (rc != GM_OK) return rc;
  gq_unpack(p->net, packed.data(), out);
  return GM_OK;
}

extern "C" {

void gm_ppo_opt_default(gm_ppo_opt* out) {
  if (!out) return;
  gm_ppo_opt o{};
  o.learning_rate_pi = 3e-4; o.learning_rate_vf = 1e-3; o.gamma = 0.99; o.lam = 0.97; o.clip_ratio = 0.2;
  o.train_pi_iters = 80; o.train_vf_iters = 80;
  o.target_kl = 0.01; o.max_kl_ratio = 1.5;
  o.optimiser = GM_OPT_ADAM;
  o.use_kl_penalty = 0; o.kl_penalty_coefficient = 0.2;
  o.use_entropy_regularisation = 0; o.entropy_coefficient = 1e-4;
  o.adam_beta1 = 0.9; o.adam_beta2 = 0.999;
  o.grad_clamp_value = 0.0;
  *out = o;
}

int gm_ac_adv_normalise(gm_ctx* c, float* adv, int64_t n) {
  if (!c) return GM_E_ARG;
  if (!adv || n < 2) return fail(c, GM_E_ARG, "gm_ac_adv_normalise: no array or n < 2 (one value has no standard deviation)");
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(gm_ac_adv_normalise_kernel, dim3(1), dim3(1024), 0, c->stream, adv, (long long)n);
  HIPCHK(c, hipGetLastError());
  return GM_OK;
}

int gm_ac_get_params(gm_ac* p, float* flat) {
  if (!p || !p->ctx || !flat) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  return ac_unpack(c, p, p->d_params, flat);
}

int gm_ac_get_packed(gm_ac* p, float* packed) {
  if (!p || !p->ctx || !packed) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  return read_back(c, packed, p->d_params, sizeof(float) * (size_t)p->total);
}

int gm_ppo_learner_create(gm_ac* ac, const gm_ppo_opt* opt, int n_groups, gm_ppo_learner** out) {
  if (!ac || !ac->ctx || !out) return GM_E_ARG;
  gm_ctx* c = ac->ctx;
  gm_ppo_opt o;
  gm_ppo_opt_default(&o);
  if (opt) o = *opt;
  if (o.optimiser != GM_OPT_ADAM && o.optimiser != GM_OPT_ADAMW)
    return fail(c, GM_E_ARG, "gm_ppo_learner_create: optimiser must be GM_OPT_ADAM / GM_OPT_ADAMW (RMSprop is not on the device)");
  if (!(o.learning_rate_pi >= 0) || !(o.learning_rate_vf >= 0) || !(o.adam_beta1 >= 0 && o.adam_beta1 < 1) ||
      !(o.adam_beta2 >= 0 && o.adam_beta2 < 1) || !(o.clip_ratio >= 0) || o.train_pi_iters < 0 || o.train_vf_iters < 0)
    return fail(c, GM_E_ARG, "gm_ppo_learner_create: learning rates, clip_ratio, iteration counts >= 0 and betas in [0, 1) expected");
  if (n_groups < 0 || n_groups > GQ_MAX_GROUPS)
    return fail(c, GM_E_ARG, "gm_ppo_learner_create: n_groups in 0 (the default) .. " + std::to_string(GQ_MAX_GROUPS) + " expected");
  HIPCHK(c, hipSetDevice(c->device));
  gm_ppo_learner* l = new gm_ppo_learner;
  l->ctx = c;
  l->ac = ac;
  l->opt = o;
  l->groups = n_groups ? n_groups : GQ_DEFAULT_GROUPS;
  l->plan_pi = gl_plan(ac->net.actor);
  l->plan_vf = gl_plan(ac->net.critic);
  const int rows = std::max(l->plan_pi.total, l->plan_vf.total);
  l->spill_stride = rows > GL_ARENA ? rows : 1;
  const size_t total = (size_t)ac->total, G = (size_t)l->groups;
  hipError_t e = l->d_partials.alloc(total * G);
  if (e == hipSuccess) e = l->d_wg.alloc(G * GQ_INFO);
  if (e == hipSuccess) e = l->d_grad.alloc(total);
  if (e == hipSuccess) e = l->d_m.alloc(total);
  if (e == hipSuccess) e = l->d_v.alloc(total);
  if (e == hipSuccess) e = l->d_vmax.alloc(total);
  if (e == hipSuccess) e = l->d_scalars.alloc(3 * GQ_SCALARS);
  if (e == hipSuccess) e = l->d_stop.alloc(2);
  if (e == hipSuccess) e = l->d_spill.alloc((size_t)l->spill_stride * (rows > GL_ARENA ? G : 1));
  for (float* z : {l->d_grad.get(), l->d_m.get(), l->d_v.get(), l->d_vmax.get()})
    if (e == hipSuccess) e = hipMemsetAsync(z, 0, sizeof(float) * total, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(l->d_scalars, 0, sizeof(float) * 3 * GQ_SCALARS, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(l->d_stop, 0, sizeof(int32_t) * 2, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    gm_ppo_learner_destroy(l);
    return fail(c, GM_E_HIP, std::string("gm_ppo_learner_create: ") + hipGetErrorString(e));
  }
  *out = l;
  return GM_OK;
}

void gm_ppo_learner_destroy(gm_ppo_learner* l) {
  if (!l) return;
  if (l->ctx) {
    (void)hipSetDevice(l->ctx->device);
    (void)hipStreamSynchronize(l->ctx->stream);   // the stream may still use the learner's buffers
  }
  delete l;
}

int gm_ppo_learner_grad_pi(gm_ppo_learner* l, const gm_ppo_batch* batch) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  if (!ppo_batch_ok(batch, true)) return fail(c, GM_E_ARG, "gm_ppo_learner_grad_pi: incomplete batch (obs, act, logp, adv) or n < 1");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, ppo_launch_grad(l, true, *batch, nullptr, nullptr, nullptr));
  return GM_OK;
}

int gm_ppo_learner_grad_vf(gm_ppo_learner* l, const gm_ppo_batch* batch) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  if (!ppo_batch_ok(batch, false)) return fail(c, GM_E_ARG, "gm_ppo_learner_grad_vf: incomplete batch (obs, ret) or n < 1");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, ppo_launch_grad(l, false, *batch, nullptr, nullptr, nullptr));
  return GM_OK;
}

int gm_ppo_learner_step_pi(gm_ppo_learner* l) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  l->step_pi++;
  HIPCHK(c, ppo_launch_step(l, true, l->step_pi, nullptr));
  return GM_OK;
}

int gm_ppo_learner_step_vf(gm_ppo_learner* l) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  l->step_vf++;
  HIPCHK(c, ppo_launch_step(l, false, l->step_vf, nullptr));
  return GM_OK;
}

int gm_ppo_learner_read(gm_ppo_learner* l, float* grad_flat, float* scalars) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  if (grad_flat) {
    const int rc = ac_unpack(c, l->ac, l->d_grad, grad_flat);
    if (rc != GM_OK) return rc;
  }
  return scalars ? read_back(c, scalars, l->d_scalars, sizeof(float) * GQ_SCALARS) : (int)GM_OK;
}

int gm_ppo_learner_get_state(gm_ppo_learner* l, int64_t* steps, float* exp_avg, float* exp_avg_sq,
                             float* max_exp_avg_sq) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  if (steps) { steps[0] = l->step_pi; steps[1] = l->step_vf; }
  const float* src[3] = {l->d_m, l->d_v, l->d_vmax};
  float* dst[3] = {exp_avg, exp_avg_sq, max_exp_avg_sq};
  for (int i = 0; i < 3; i++)
    if (dst[i]) {
      const int rc = ac_unpack(c, l->ac, src[i], dst[i]);
      if (rc != GM_OK) return rc;
    }
  return GM_OK;
}

int gm_ppo_learner_set_state(gm_ppo_learner* l, const int64_t* steps, const float* exp_avg, const float* exp_avg_sq,
                             const float* max_exp_avg_sq) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  if (steps && (steps[0] < 0 || steps[1] < 0)) return fail(c, GM_E_ARG, "gm_ppo_learner_set_state: negative step");
  HIPCHK(c, hipSetDevice(c->device));
  const float* src[3] = {exp_avg, exp_avg_sq, max_exp_avg_sq};
  float* dst[3] = {l->d_m, l->d_v, l->d_vmax};
  std::vector<float> packed((size_t)l->ac->total);
  for (int i = 0; i < 3; i++)
    if (src[i]) {
      gq_pack(l->ac->net, l->ac->total, src[i], packed.data());
      const int rc = stage_upload(c, dst[i], packed.data(), sizeof(float) * packed.size());
      if (rc != GM_OK) return rc;
    }
  if (steps) { l->step_pi = steps[0]; l->step_vf = steps[1]; }
  return GM_OK;
}

int gm_ppo_learner_update(gm_ppo_learner* l, const gm_ac_traj* traj, int n_steps, gm_ppo_info* info) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  if (!ac_traj_ok(traj) || n_steps < 1 || n_steps > traj->capacity)
    return fail(c, GM_E_ARG, "gm_ppo_learner_update: incomplete trajectory buffer or n_steps outside its capacity");
  const size_t rows = (size_t)n_steps * (size_t)c->n_envs;
  if (rows < 2) return fail(c, GM_E_ARG, "gm_ppo_learner_update: one row has no standard deviation to normalise with");
  HIPCHK(c, hipSetDevice(c->device));
  if (rows > l->rows_cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, l->d_adv.alloc(rows));
    HIPCHK(c, l->d_ret.alloc(rows));
    l->rows_cap = rows;
  }
  int rc = gm_ac_gae(c, traj, n_steps, (float)l->opt.gamma, (float)l->opt.lam, l->d_adv, l->d_ret);
  if (rc == GM_OK) rc = gm_ac_adv_normalise(c, l->d_adv, (int64_t)rows);
  if (rc != GM_OK) return rc;
  const gm_ppo_batch b{(int64_t)rows, traj->obs, traj->act, traj->logp, l->d_adv, l->d_ret};
  float* first = l->d_scalars + GQ_SCALARS;
  float* last = l->d_scalars + 2 * GQ_SCALARS;
  HIPCHK(c, hipMemsetAsync(l->d_stop, 0, sizeof(int32_t) * 2, c->stream));
  HIPCHK(c, hipMemsetAsync(first, 0, sizeof(float) * 2 * GQ_SCALARS, c->stream));
  // the stop latches, so iteration i's step, if taken at all, is optimiser step step_pi + i + 1
  for (int i = 0; i < l->opt.train_pi_iters; i++) {
    HIPCHK(c, ppo_launch_grad(l, true, b, l->d_stop, i == 0 ? first : nullptr, last));
    HIPCHK(c, ppo_launch_step(l, true, l->step_pi + i + 1, l->d_stop));
  }
  for (int i = 0; i < l->opt.train_vf_iters; i++) {
    HIPCHK(c, ppo_launch_grad(l, false, b, nullptr, i == 0 ? first : nullptr, last));
    HIPCHK(c, ppo_launch_step(l, false, l->step_vf + i + 1, nullptr));
  }
  // the one host read: the latch's step count and the info rows
  struct { int32_t stop[2]; float rows[2 * GQ_SCALARS]; } h;
  HIPCHK(c, hipMemcpyAsync(h.stop, l->d_stop, sizeof(h.stop), hipMemcpyDeviceToHost, c->stream));
  rc = read_back(c, h.rows, first, sizeof(h.rows));
  if (rc != GM_OK) return rc;
  l->step_pi += h.stop[1];
  l->step_vf += l->opt.train_vf_iters;
  if (info) {
    info->pi_iters_done = h.stop[1];
    info->pad = 0;
    std::memcpy(info->first, h.rows, sizeof(float) * GQ_SCALARS);
    std::memcpy(info->last, h.rows + GQ_SCALARS, sizeof(float) * GQ_SCALARS);
  }
  return GM_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- on-device SAC (collection side)
struct gm_sac {
  gm_ctx* ctx = nullptr;
  GsNet net{};
  int64_t total = 0;           // packed floats
  int64_t n_raw = 0;           // floats of the caller's (parameters() order) parameters
  std::vector<int32_t> pisz, qsz;
  DevBuf<float> d_params;
  // what gm_sac_act leaves (gm_sac_read): [n_envs][n_act] each, logp [n_envs]
  DevBuf<float> d_act, d_logp, d_u, d_mu, d_ls;
  DevBuf<GsArgs> d_args;       // gm_sac_rollout's launch arguments
  DevBuf<GrArgs> d_rep;        // and its memory as replay_record's second half sees it
  // gm_sac_target's a2 and logp2 where the caller keeps none (grown on demand)
  DevBuf<float> d_ta2, d_tlogp;
  int t_cap = 0;
};

// the layout of [pi | q1 | q2] for pi_sizes = [n_obs, *hidden, n_act] and q_sizes: the packed
// float count, or -1; head: pi's sizes with the stacked output layer
static int64_t sac_layout(const int32_t* pisz, int npi, const int32_t* qsz, int nq, GsNet* net, int64_t* n_raw,
                          std::vector<int32_t>* head) {
  if (!pisz || !qsz || npi < 2 || nq < 2) return -1;
  const int na = pisz[npi - 1];
  if (na < 1 || na > GA_MAX_ACT || qsz[0] != pisz[0] + na || qsz[nq - 1] != 1) return -1;
  std::vector<int32_t> h(pisz, pisz + npi);
  h[npi - 1] = 2 * na;
  GsNet N{};
  const int64_t tp = gl_layout(h.data(), npi, &N.pi);
  const int64_t tq = gl_layout(qsz, nq, &N.q);
  if (tp < 0 || tq < 0) return -1;
  N.n_act = na;
  N.q1_off = tp;
  N.q2_off = tp + tq;
  if (net) *net = N;
  if (n_raw) *n_raw = gl_flat_count(N.pi) + 2 * gl_flat_count(N.q);
  if (head) *head = h;
  return tp + 2 * tq;
}
static bool sac_replay_ok(const gm_sac_replay* r) {
  return r && r->capacity >= 1 && r->state && r->action && r->next_state && r->reward && r->end;
}
// the two device views of a caller's memory for a call of n_steps env-steps that starts after
// row0 pushed transitions (G: state and action rows; R: replay_record's / the DQN push's view,
// its action NULL); false with the message what for a memory the call cannot use
static bool sac_replay_args(gm_ctx* c, const gm_sac_replay* r, int64_t row0, int n_steps, const char* what, GsReplay& G,
                            GrArgs& R) {
  if (!sac_replay_ok(r) || row0 < 0) {
    fail(c, GM_E_ARG, std::string(what) + ": incomplete replay memory or negative row0");
    return false;
  }
  if ((int64_t)n_steps * c->n_envs > r->capacity) {
    fail(c, GM_E_ARG, std::string(what) + ": " + std::to_string(n_steps) + " env-steps of " + std::to_string(c->n_envs) +
                          " envs would write a row of the replay memory twice (capacity " +
                          std::to_string((long long)r->capacity) + ")");
    return false;
  }
  const long long r0 = (long long)(row0 % r->capacity);
  G = GsReplay{r->state, r->action, (long long)r->capacity, r0};
  R = GrArgs{r->state, nullptr, r->next_state, r->reward, r->end, (long long)r->capacity, r0, c->cfg.n_obs, 0};
  return true;
}
static hipError_t sac_launch_actor(gm_ctx* c, const gm_sac* p, const float* obs, int n, long long id0, int mode,
                                   uint64_t seed, uint64_t decision, const GsActOut& out) {
  hipLaunchKernelGGL(gm_sac_actor_kernel, dim3((n + GP_TILE - 1) / GP_TILE), dim3(64), 0, c->stream, obs, n, id0,
                     p->d_params.get(), p->net, mode, seed, decision, out);
  return hipGetLastError();
}
static bool sac_mode_ok(int mode) { return mode == GM_SAC_MEAN || mode == GM_SAC_SAMPLE || mode == GM_SAC_RANDOM; }

extern "C" {

void gm_sac_opt_default(gm_sac_opt* out) {
  if (!out) return;
  *out = gm_sac_opt{GP_ACT_RELU, 1.0f, -20.0f, 2.0f};
}

int64_t gm_sac_struct_size(int which) {
  switch (which) {
    case 0: return (int64_t)sizeof(gm_sac_replay);
    case 1: return (int64_t)sizeof(gm_sac_batch);
    case 2: return (int64_t)sizeof(gm_sac_opt);
    case 4: return (int64_t)sizeof(gm_sac_learn_opt);
    default: return -1;
  }
}

int64_t gm_sac_pack(const int32_t* pi_sizes, int n_pi, const int32_t* q_sizes, int n_q, int activation,
                    const float* params, float* out, int64_t* offsets) {
  GsNet N;
  std::vector<int32_t> head;
  if (activation != GP_ACT_RELU && activation != GP_ACT_TANH) return -1;
  const int64_t total = sac_layout(pi_sizes, n_pi, q_sizes, n_q, &N, nullptr, &head);
  if (total < 0) return total;
  if (offsets) { offsets[0] = N.q1_off; offsets[1] = N.q2_off; }
  if (!out) return total;
  if (!params) return GM_E_ARG;
  // the flat order already is the stacked layer's: mu_layer.W, mu_layer.b, log_std_layer.W,
  // log_std_layer.b -> W = [mu W; log_std W] [2 n_act x in], b = [mu b; log_std b]
  const int na = N.n_act, hin = pi_sizes[n_pi - 2];
  int64_t hidden = 0;
  for (int l = 0; l + 2 < n_pi; l++) hidden += (int64_t)pi_sizes[l + 1] * pi_sizes[l] + pi_sizes[l + 1];
  std::vector<float> pi((size_t)gl_flat_count(N.pi));
  std::memcpy(pi.data(), params, sizeof(float) * (size_t)hidden);
  const float* mu_w = params + hidden;
  const float* mu_b = mu_w + (size_t)na * hin;
  const float* ls_w = mu_b + na;
  const float* ls_b = ls_w + (size_t)na * hin;
  float* w = pi.data() + hidden;
  std::memcpy(w, mu_w, sizeof(float) * (size_t)na * hin);
  std::memcpy(w + (size_t)na * hin, ls_w, sizeof(float) * (size_t)na * hin);
  std::memcpy(w + (size_t)2 * na * hin, mu_b, sizeof(float) * (size_t)na);
  std::memcpy(w + (size_t)2 * na * hin + na, ls_b, sizeof(float) * (size_t)na);
  gm_policy_pack(head.data(), n_pi, pi.data(), out);
  const float* q = params + gl_flat_count(N.pi);
  gm_policy_pack(q_sizes, n_q, q, out + N.q1_off);
  gm_policy_pack(q_sizes, n_q, q + gl_flat_count(N.q), out + N.q2_off);
  return total;
}

int gm_sac_create(gm_ctx* c, const int32_t* pi_sizes, int n_pi, const int32_t* q_sizes, int n_q, const gm_sac_opt* opt,
                  const float* params, gm_sac** out) {
  if (!c || !pi_sizes || !q_sizes || !params || !out || n_pi < 2 || n_q < 2) return GM_E_ARG;
  gm_sac_opt o;
  gm_sac_opt_default(&o);
  if (opt) o = *opt;
  if (o.activation != GP_ACT_RELU && o.activation != GP_ACT_TANH)
    return fail(c, GM_E_ARG, "gm_sac_create: activation must be 0 (ReLU) or 1 (Tanh)");
  if (!(o.action_limit > 0.0f) || !(o.log_std_min <= o.log_std_max))
    return fail(c, GM_E_ARG, "gm_sac_create: action_limit > 0 and log_std_min <= log_std_max expected");
  GsNet N;
  int64_t n_raw = 0;
  const int64_t total = sac_layout(pi_sizes, n_pi, q_sizes, n_q, &N, &n_raw, nullptr);
  if (total < 0)
    return fail(c, GM_E_ARG, "gm_sac_create: <= 8 layers of width 1..256, n_actions <= " + std::to_string(GA_MAX_ACT) +
                                 " and critics that map n_obs + n_actions to 1 expected");
  if (!c->cfg.s.continous_actions)
    return fail(c, GM_E_ARG, "gm_sac_create: the squashed Gaussian actor needs continuous actions (continous_actions != 0)");
  if (N.pi.width[0] != c->cfg.n_obs || N.n_act != c->cfg.n_actions)
    return fail(c, GM_E_ARG, "gm_sac_create: the actor must map n_obs (" + std::to_string(c->cfg.n_obs) +
                                 ") to n_actions (" + std::to_string(c->cfg.n_actions) + ")");
  N.act = o.activation;
  N.limit = o.action_limit;
  N.ls_min = o.log_std_min;
  N.ls_max = o.log_std_max;
  HIPCHK(c, hipSetDevice(c->device));
  gm_sac* p = new gm_sac;
  p->ctx = c;
  p->net = N;
  p->total = total;
  p->n_raw = n_raw;
  p->pisz.assign(pi_sizes, pi_sizes + n_pi);
  p->qsz.assign(q_sizes, q_sizes + n_q);
  const size_t rows = (size_t)c->n_envs * N.n_act;
  hipError_t e = p->d_params.alloc((size_t)total);
  if (e == hipSuccess) e = p->d_args.alloc(1);
  if (e == hipSuccess) e = p->d_rep.alloc(1);
  if (e == hipSuccess) e = p->d_act.alloc(rows);
  if (e == hipSuccess) e = p->d_u.alloc(rows);
  if (e == hipSuccess) e = p->d_mu.alloc(rows);
  if (e == hipSuccess) e = p->d_ls.alloc(rows);
  if (e == hipSuccess) e = p->d_logp.alloc((size_t)c->n_envs);
  if (e != hipSuccess) {
    gm_sac_destroy(p);
    return fail(c, GM_E_HIP, std::string("gm_sac_create: ") + hipGetErrorString(e));
  }
  const int rc = gm_sac_set_params(p, params);
  if (rc != GM_OK) { gm_sac_destroy(p); return rc; }
  *out = p;
  return GM_OK;
}

void gm_sac_destroy(gm_sac* p) {
  if (!p) return;
  if (p->ctx) {
    (void)hipSetDevice(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);
  }
  delete p;
}

int gm_sac_set_params(gm_sac* p, const float* params) {
  if (!p || !p->ctx || !params) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<float> packed((size_t)p->total);
  gm_sac_pack(p->pisz.data(), (int)p->pisz.size(), p->qsz.data(), (int)p->qsz.size(), p->net.act, params,
              packed.data(), nullptr);
  return stage_upload(c, p->d_params, packed.data(), sizeof(float) * (size_t)p->total);
}

int gm_sac_get_packed(gm_sac* p, float* packed) {
  if (!p || !p->ctx || !packed) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  return read_back(c, packed, p->d_params, sizeof(float) * (size_t)p->total);
}

int gm_sac_get_params(gm_sac* p, float* flat) {
  if (!p || !p->ctx || !flat) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  std::vector<float> packed((size_t)p->total);
  const int rc = gm_sac_get_packed(p, packed.data());
  if (rc != GM_OK) return rc;
  // the inverse of gm_sac_pack: the stacked head back into mu_layer and log_std_layer
  const GsNet& N = p->net;
  const int na = N.n_act, L = N.pi.n_layers, hin = N.pi.width[L - 1];
  int64_t hidden = 0;
  for (int l = 0; l + 1 < L; l++) hidden += (int64_t)N.pi.width[l + 1] * N.pi.width[l] + N.pi.width[l + 1];
  std::vector<float> pi((size_t)gl_flat_count(N.pi));
  gl_for_each_param(N.pi, [&](int64_t i, int64_t k) { pi[(size_t)i] = packed[(size_t)k]; });
  std::memcpy(flat, pi.data(), sizeof(float) * (size_t)hidden);
  const float* w = pi.data() + hidden;
  float* dst = flat + hidden;
  std::memcpy(dst, w, sizeof(float) * (size_t)na * hin);                                        // mu_layer.W
  std::memcpy(dst + (size_t)na * hin, w + (size_t)2 * na * hin, sizeof(float) * (size_t)na);    // mu_layer.b
  std::memcpy(dst + (size_t)na * hin + na, w + (size_t)na * hin, sizeof(float) * (size_t)na * hin);       // log_std_layer.W
  std::memcpy(dst + (size_t)2 * na * hin + na, w + (size_t)2 * na * hin + na, sizeof(float) * (size_t)na);   // .b
  float* q = flat + gl_flat_count(N.pi);
  const int64_t nq = gl_flat_count(N.q);
  gl_for_each_param(N.q, [&](int64_t i, int64_t k) {
    q[(size_t)i] = packed[(size_t)(N.q1_off + k)];
    q[(size_t)(nq + i)] = packed[(size_t)(N.q2_off + k)];
  });
  return GM_OK;
}

int gm_sac_act(gm_sac* p, int mode, uint64_t seed, uint64_t decision) {
  if (!p || !p->ctx) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  if (!sac_mode_ok(mode)) return fail(c, GM_E_ARG, "gm_sac_act: mode must be GM_SAC_MEAN, GM_SAC_SAMPLE or GM_SAC_RANDOM");
  HIPCHK(c, hipSetDevice(c->device));
  const GsActOut out{p->d_act, p->d_logp, p->d_u, p->d_mu, p->d_ls};
  HIPCHK(c, sac_launch_actor(c, p, c->d_obs, c->n_envs, c->env_offset, mode, seed, decision, out));
  return gm_set_action(c, p->d_act, 1);
}

int gm_sac_read(gm_sac* p, float* act, float* logp, float* u, float* mu, float* log_std) {
  if (!p || !p->ctx) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t rows = sizeof(float) * (size_t)c->n_envs * p->net.n_act;
  const struct { float* dst; const float* src; size_t bytes; } cp[] = {
      {act, p->d_act, rows}, {logp, p->d_logp, sizeof(float) * (size_t)c->n_envs}, {u, p->d_u, rows},
      {mu, p->d_mu, rows}, {log_std, p->d_ls, rows}};
  for (const auto& x : cp)
    if (x.dst) HIPCHK(c, hipMemcpyAsync(x.dst, x.src, x.bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GM_OK;
}

int gm_sac_push_begin(gm_sac* p, const gm_sac_replay* replay, int64_t row0) {
  if (!p || !p->ctx) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  GsReplay G;
  GrArgs R;
  if (!sac_replay_args(c, replay, row0, 1, "gm_sac_push_begin", G, R)) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, launch_per_obs_element(c, (long long)c->n_envs * c->cfg.n_obs, gm_sac_push_begin_kernel, c->d_obs,
                                   p->d_act.get(), c->n_envs, c->cfg.n_obs, p->net.n_act, G));
  return GM_OK;
}

int gm_sac_push_end(gm_sac* p, const gm_sac_replay* replay, int64_t row0, int max_episode_steps) {
  if (!p || !p->ctx) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  GsReplay G;
  GrArgs R;
  if (!sac_replay_args(c, replay, row0, 1, "gm_sac_push_end", G, R)) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  // (the DQN memory's second half: it writes next_state, reward and end, no action)
  HIPCHK(c, launch_per_obs_element(c, (long long)c->n_envs * c->cfg.n_obs, gm_replay_push_end_kernel, c->d_obs,
                                   c->d_state.get(), c->d_rew, c->d_done, c->n_envs, max_episode_steps, R));
  return GM_OK;
}

int gm_sac_rollout(gm_sac* p, int n_steps, int mode, uint64_t seed, uint64_t decision0, int max_episode_steps,
                   gm_episode_end* records, const gm_sac_replay* replay, int64_t row0) {
  if (!p || !p->ctx) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  if (n_steps < 1 || !sac_mode_ok(mode))
    return fail(c, GM_E_ARG, "gm_sac_rollout: n_steps >= 1 and mode GM_SAC_MEAN, GM_SAC_SAMPLE or GM_SAC_RANDOM expected");
  GsReplay G{};
  GrArgs R{};
  if (replay && !sac_replay_args(c, replay, row0, n_steps, "gm_sac_rollout", G, R)) return GM_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (chunk_queue_on(c)) {
    GsArgs A{};
    A.net = p->net;
    A.params = p->d_params;
    A.rep = G;
    A.mode = mode;
    A.seed = seed;
    A.decision0 = decision0;
    int rc = stage_upload(c, p->d_args, &A, sizeof(GsArgs));
    if (rc == GM_OK && replay) rc = stage_upload(c, p->d_rep, &R, sizeof(GrArgs));
    if (rc != GM_OK) return rc;
    GmRolloutJob job = rollout_job(c, n_steps, GM_DRV_SAC, seed, 0.0f, max_episode_steps, records);
    job.sac = p->d_args;
    job.replay = replay ? p->d_rep.get() : nullptr;
    return timed_launch(c, &job);
  }
  return per_step_rollout(
      c, n_steps, max_episode_steps, records,
      [&](int k) {
        const int rc = gm_sac_act(p, mode, seed, decision0 + (uint64_t)k);
        return rc == GM_OK && replay ? gm_sac_push_begin(p, replay, row0 + (int64_t)k * c->n_envs) : rc;
      },
      [&](int k) {
        return replay ? gm_sac_push_end(p, replay, row0 + (int64_t)k * c->n_envs, max_episode_steps) : (int)GM_OK;
      });
}

int gm_sac_evaluate(gm_sac* p, int mode, uint64_t seed, uint64_t decision0, int max_episode_steps,
                    const uint8_t* active, const gm_eval_out* out) {
  if (!p || !p->ctx) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  if (!sac_mode_ok(mode))
    return fail(c, GM_E_ARG, "gm_sac_evaluate: mode must be GM_SAC_MEAN, GM_SAC_SAMPLE or GM_SAC_RANDOM");
  int rc = eval_action_kind(c, "gm_sac_evaluate", true, "the SAC actor");
  if (rc == GM_OK) rc = eval_check(c, "gm_sac_evaluate", max_episode_steps, out);
  if (rc != GM_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (chunk_queue_on(c)) {
    GsArgs A{};   // (rep.state == NULL: the driver records nothing)
    A.net = p->net;
    A.params = p->d_params;
    A.mode = mode;
    A.seed = seed;
    A.decision0 = decision0;
    rc = stage_upload(c, p->d_args, &A, sizeof(GsArgs));
    if (rc != GM_OK) return rc;
    GmRolloutJob job = rollout_job(c, max_episode_steps, GM_DRV_SAC, seed, 0.0f, max_episode_steps, nullptr);
    job.sac = p->d_args;
    return eval_launch(c, job, active, out);
  }
  return per_step_evaluate(c, max_episode_steps, active, out,
                           [&](int k) { return gm_sac_act(p, mode, seed, decision0 + (uint64_t)k); });
}

int gm_sac_replay_sample(gm_ctx* c, const gm_sac_replay* replay, int64_t size, int batch, uint64_t seed, uint64_t draw,
                         const gm_sac_batch* out) {
  if (!c) return GM_E_ARG;
  if (!sac_replay_ok(replay) || !out || !out->state || !out->action || !out->next_state || !out->reward || !out->end ||
      !out->index)
    return fail(c, GM_E_ARG, "gm_sac_replay_sample: incomplete replay memory or batch arrays");
  if (size < 1 || size > replay->capacity || size > 0x7FFFFFFFll || batch < 1 || batch > size)
    return fail(c, GM_E_ARG, "gm_sac_replay_sample: batch " + std::to_string(batch) + " of " +
                                 std::to_string((long long)size) + " stored transitions (capacity " +
                                 std::to_string((long long)replay->capacity) + "): 1 <= batch <= size <= capacity expected");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, launch_per_obs_element(c, (long long)batch * c->cfg.n_obs, gm_sac_replay_sample_kernel, *replay,
                                   c->cfg.n_obs, c->cfg.n_actions, (long long)size, batch, gr_key(seed, draw), *out));
  return GM_OK;
}

int gm_sac_q(gm_sac* p, const float* state, const float* action, int n, float* q1, float* q2) {
  if (!p || !p->ctx) return GM_E_ARG;
  gm_ctx* c = p->ctx;
  if (!state || !action || n < 1) return fail(c, GM_E_ARG, "gm_sac_q: no state or action array, or n < 1");
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(gm_sac_q_kernel, dim3((n + GP_TILE - 1) / GP_TILE), dim3(64), 0, c->stream, state, action, n,
                     p->d_params.get(), p->net, q1, q2, GsBackup{});
  HIPCHK(c, hipGetLastError());
  return GM_OK;
}

int gm_sac_target(gm_sac* target, gm_sac* online, const gm_sac_batch* batch, int n, float gamma, float alpha,
                  int bootstrap_truncated, uint64_t seed, uint64_t draw, float* y, float* a2, float* u2, float* logp2,
                  float* qmin) {
  if (!target || !target->ctx || !online) return GM_E_ARG;
  gm_ctx* c = target->ctx;
  if (online->ctx != c) return fail(c, GM_E_ARG, "gm_sac_target: the two handles belong to different contexts");
  if (online->pisz != target->pisz || online->qsz != target->qsz)
    return fail(c, GM_E_ARG, "gm_sac_target: the two handles have different network sizes");
  if (!batch || !batch->next_state || !batch->reward || !batch->end || !y || n < 1)
    return fail(c, GM_E_ARG, "gm_sac_target: incomplete batch (next_state, reward, end), no y or n < 1");
  HIPCHK(c, hipSetDevice(c->device));
  const int na = target->net.n_act;
  if ((!a2 || !logp2) && n > target->t_cap) {
    // (the stream may still read the old arrays: wait before freeing them)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    target->t_cap = 0;
    HIPCHK(c, target->d_ta2.alloc((size_t)n * na));
    HIPCHK(c, target->d_tlogp.alloc((size_t)n));
    target->t_cap = n;
  }
  float* a = a2 ? a2 : target->d_ta2.get();
  float* lp = logp2 ? logp2 : target->d_tlogp.get();
  HIPCHK(c, sac_launch_actor(c, online, batch->next_state, n, 0, GM_SAC_SAMPLE, seed, draw,
                             GsActOut{a, lp, u2, nullptr, nullptr}));
  const GsBackup B{batch->reward, batch->end, lp, gamma, alpha, bootstrap_truncated, 0, y, qmin};
  hipLaunchKernelGGL(gm_sac_q_kernel, dim3((n + GP_TILE - 1) / GP_TILE), dim3(64), 0, c->stream, batch->next_state,
                     (const float*)a, n, target->d_params.get(), target->net, (float*)nullptr, (float*)nullptr, B);
  HIPCHK(c, hipGetLastError());
  return GM_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- on-device SAC learner
struct gm_sac_learner {
  gm_ctx* ctx = nullptr;
  gm_sac* online = nullptr;
  gm_sac_learn_opt opt{};
  GlPlan plan_pi{}, plan_q{};
  int64_t step_q = 0, step_pi = 0;   // optimiser steps taken
  int64_t pi_total = 0, q_total = 0; // packed floats of the actor and of one critic
  DevBuf<float> d_part_q;       // [GL_MAX_TILES][2 q_total] per-tile gradients of [q1 | q2]
  DevBuf<float> d_part_pi;      // [GL_MAX_TILES][pi_total]
  DevBuf<float> d_tile_loss;    // [3][GL_MAX_TILES]: q1, q2, pi
  DevBuf<float> d_grad, d_m, d_v, d_vmax;   // [blob], packed order: both optimisers' ranges
  DevBuf<float> d_loss;         // [2] loss_q, loss_pi of the held gradients
  DevBuf<float> d_spill_q, d_spill_pi;      // the gradient kernels' rows where they do not fit LDS
  // gm_sac_learner_train's batch and backup
  DevBuf<float> d_state, d_action, d_next, d_reward, d_y;
  DevBuf<int32_t> d_index;
  DevBuf<uint8_t> d_end;
};

static gm_dqn_opt sac_learner_dqn_opt(const gm_sac_learn_opt& o) {   // (learner_opt's input; SAC has no clamp)
  return gm_dqn_opt{o.optimiser, o.amsgrad, GM_LOSS_MSE, 0, o.lr, o.beta1, o.beta2, o.eps, o.weight_decay, 0.0};
}
// One launch of gm_learn_step_kernel over one optimiser's range of the blob: the critics'
// [q1 | q2] or the actor's [pi].  target: the handle whose same range is polyak-updated, or NULL.
static hipError_t sac_launch_step(gm_sac_learner* l, bool critics, bool sum, bool step, gm_sac* target, float tau, int n,
                                  float* loss_out) {
  gm_ctx* c = l->ctx;
  const long long off = critics ? l->online->net.q1_off : 0;
  GlStepArgs a{};
  a.do_sum = sum;
  a.do_step = step;
  a.do_soft = target != nullptr;
  a.n_tiles = (n + GP_TILE - 1) / GP_TILE;
  a.n = n;
  a.total = critics ? 2 * (long long)l->q_total : (long long)l->pi_total;
  a.partials = critics ? l->d_part_q.get() : l->d_part_pi.get();
  a.tile_loss = l->d_tile_loss.get() + (critics ? 0 : 2 * GL_MAX_TILES);
  a.tile_loss2 = critics ? l->d_tile_loss.get() + GL_MAX_TILES : nullptr;
  a.grad = l->d_grad.get() + off;
  a.loss = l->d_loss.get() + (critics ? 0 : 1);
  a.loss_out = loss_out;
  a.p = l->online->d_params.get() + off;
  a.m = l->d_m.get() + off;
  a.v = l->d_v.get() + off;
  a.vmax = l->d_vmax.get() + off;
  a.target = target ? target->d_params.get() + off : nullptr;
  a.tau = tau;
  a.opt = learner_opt(sac_learner_dqn_opt(l->opt), std::max<int64_t>(critics ? l->step_q : l->step_pi, 1));
  const int threads = 256;
  hipLaunchKernelGGL(gm_learn_step_kernel, dim3((unsigned)((a.total + threads - 1) / threads)), dim3(threads), 0,
                     c->stream, a);
  return hipGetLastError();
}
static hipError_t sac_launch_grad_q(gm_sac_learner* l, const float* state, const float* action, const float* y, int n) {
  gm_sac* p = l->online;
  GslQArgs a{};
  a.state = state;
  a.action = action;
  a.y = y;
  a.n = n;
  a.params = p->d_params;
  a.net = p->net;
  a.plan = l->plan_q;
  a.spill = l->d_spill_q;
  a.partials = l->d_part_q;
  a.q_total = (long long)l->q_total;
  a.tile_loss = l->d_tile_loss;
  const dim3 grid((n + GP_TILE - 1) / GP_TILE, 2);
  if (p->net.act == GP_ACT_TANH) hipLaunchKernelGGL(gm_sac_grad_q_kernel<GP_ACT_TANH>, grid, dim3(64), 0, l->ctx->stream, a);
  else hipLaunchKernelGGL(gm_sac_grad_q_kernel<GP_ACT_RELU>, grid, dim3(64), 0, l->ctx->stream, a);
  return hipGetLastError();
}
static hipError_t sac_launch_grad_pi(gm_sac_learner* l, const float* state, int n, float alpha, uint64_t seed,
                                     uint64_t draw, float* z, float* u, float* act, float* logp, float* q1, float* q2) {
  gm_sac* p = l->online;
  GslPiArgs a{};
  a.state = state;
  a.n = n;
  a.params = p->d_params;
  a.net = p->net;
  a.plan_pi = l->plan_pi;
  a.plan_q = l->plan_q;
  a.spill = l->d_spill_pi;
  a.partials = l->d_part_pi;
  a.pi_total = (long long)l->pi_total;
  a.tile_loss = l->d_tile_loss.get() + 2 * GL_MAX_TILES;
  a.alpha = alpha;
  a.seed = seed;
  a.draw = draw;
  a.z = z; a.u = u; a.a = act; a.logp = logp; a.q1 = q1; a.q2 = q2;
  const dim3 grid((n + GP_TILE - 1) / GP_TILE);
  if (p->net.act == GP_ACT_TANH) hipLaunchKernelGGL(gm_sac_grad_pi_kernel<GP_ACT_TANH>, grid, dim3(64), 0, l->ctx->stream, a);
  else hipLaunchKernelGGL(gm_sac_grad_pi_kernel<GP_ACT_RELU>, grid, dim3(64), 0, l->ctx->stream, a);
  return hipGetLastError();
}
static bool sac_same_sizes(const gm_sac* a, const gm_sac* b) { return a->pisz == b->pisz && a->qsz == b->qsz; }
// packed device array [blob] -> flat host array (out) through one copy
static int sac_learner_unpack(gm_ctx* c, const gm_sac* p, const float* d_packed, float* out) {
  std::vector<float> packed((size_t)p->total);
  const int rc = read_back(c, packed.data(), d_packed, sizeof(float) * (size_t)p->total);
  if (rc != GM_OK) return rc;
  gsl_unpack(p->net, packed.data(), out);
  return GM_OK;
}
static int sac_batch_check(gm_ctx* c, const char* what, int n) {
  if (n < 1) return fail(c, GM_E_ARG, std::string(what) + ": n < 1");
  if (n > GL_MAX_BATCH)
    return fail(c, GM_E_ARG, std::string(what) + ": " + std::to_string(n) + " rows, the learner holds " +
                                 std::to_string(GL_MAX_BATCH));
  return GM_OK;
}

extern "C" {

void gm_sac_learn_opt_default(gm_sac_learn_opt* out) {
  if (!out) return;
  *out = gm_sac_learn_opt{GM_OPT_ADAM, 0, 1e-4, 0.9, 0.999, 1e-8, 0.0};
}

int gm_sac_learner_create(gm_sac* online, const gm_sac_learn_opt* opt, gm_sac_learner** out) {
  if (!online || !online->ctx || !out) return GM_E_ARG;
  gm_ctx* c = online->ctx;
  gm_sac_learn_opt o;
  gm_sac_learn_opt_default(&o);
  if (opt) o = *opt;
  if (o.optimiser != GM_OPT_ADAM && o.optimiser != GM_OPT_ADAMW)
    return fail(c, GM_E_ARG, "gm_sac_learner_create: optimiser must be GM_OPT_ADAM / GM_OPT_ADAMW");
  if (!(o.lr >= 0) || !(o.beta1 >= 0 && o.beta1 < 1) || !(o.beta2 >= 0 && o.beta2 < 1) || !(o.eps >= 0) || !(o.weight_decay >= 0))
    return fail(c, GM_E_ARG, "gm_sac_learner_create: lr, eps, weight_decay >= 0 and betas in [0, 1) expected");
  HIPCHK(c, hipSetDevice(c->device));
  gm_sac_learner* l = new gm_sac_learner;
  l->ctx = c;
  l->online = online;
  l->opt = o;
  l->plan_pi = gl_plan(online->net.pi);
  l->plan_q = gl_plan(online->net.q);
  l->pi_total = online->net.q1_off;
  l->q_total = online->net.q2_off - online->net.q1_off;
  const size_t total = (size_t)online->total, n_obs = (size_t)c->cfg.n_obs, na = (size_t)online->net.n_act;
  const long long pi_rows = gsl_pi_rows(l->plan_pi, l->plan_q);
  hipError_t e = l->d_part_q.alloc(2 * (size_t)l->q_total * GL_MAX_TILES);
  if (e == hipSuccess) e = l->d_part_pi.alloc((size_t)l->pi_total * GL_MAX_TILES);
  if (e == hipSuccess) e = l->d_tile_loss.alloc(3 * GL_MAX_TILES);
  if (e == hipSuccess) e = l->d_grad.alloc(total);
  if (e == hipSuccess) e = l->d_m.alloc(total);
  if (e == hipSuccess) e = l->d_v.alloc(total);
  if (e == hipSuccess) e = l->d_vmax.alloc(total);
  if (e == hipSuccess) e = l->d_loss.alloc(2);
  if (e == hipSuccess) e = l->d_spill_q.alloc(l->plan_q.total > GL_ARENA ? (size_t)l->plan_q.total * 2 * GL_MAX_TILES : 1);
  if (e == hipSuccess) e = l->d_spill_pi.alloc(pi_rows > GL_ARENA ? (size_t)pi_rows * GL_MAX_TILES : 1);
  if (e == hipSuccess) e = l->d_state.alloc(n_obs * GL_MAX_BATCH);
  if (e == hipSuccess) e = l->d_action.alloc(na * GL_MAX_BATCH);
  if (e == hipSuccess) e = l->d_next.alloc(n_obs * GL_MAX_BATCH);
  if (e == hipSuccess) e = l->d_reward.alloc(GL_MAX_BATCH);
  if (e == hipSuccess) e = l->d_y.alloc(GL_MAX_BATCH);
  if (e == hipSuccess) e = l->d_index.alloc(GL_MAX_BATCH);
  if (e == hipSuccess) e = l->d_end.alloc(GL_MAX_BATCH);
  for (float* z : {l->d_grad.get(), l->d_m.get(), l->d_v.get(), l->d_vmax.get()})
    if (e == hipSuccess) e = hipMemsetAsync(z, 0, sizeof(float) * total, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(l->d_loss, 0, 2 * sizeof(float), c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    gm_sac_learner_destroy(l);
    return fail(c, GM_E_HIP, std::string("gm_sac_learner_create: ") + hipGetErrorString(e));
  }
  *out = l;
  return GM_OK;
}

void gm_sac_learner_destroy(gm_sac_learner* l) {
  if (!l) return;
  if (l->ctx) {
    (void)hipSetDevice(l->ctx->device);
    (void)hipStreamSynchronize(l->ctx->stream);   // the stream may still use the learner's buffers
  }
  delete l;
}

int gm_sac_learner_grad_q(gm_sac_learner* l, const gm_sac_batch* batch, const float* y, int n) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  const int rc = sac_batch_check(c, "gm_sac_learner_grad_q", n);
  if (rc != GM_OK) return rc;
  if (!batch || !batch->state || !batch->action || !y)
    return fail(c, GM_E_ARG, "gm_sac_learner_grad_q: incomplete batch (state, action) or no y");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, sac_launch_grad_q(l, batch->state, batch->action, y, n));
  HIPCHK(c, sac_launch_step(l, true, true, false, nullptr, 0.0f, n, nullptr));
  return GM_OK;
}

int gm_sac_learner_grad_pi(gm_sac_learner* l, const gm_sac_batch* batch, int n, float alpha, uint64_t seed, uint64_t draw,
                           float* z, float* u, float* a, float* logp, float* q1, float* q2) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  const int rc = sac_batch_check(c, "gm_sac_learner_grad_pi", n);
  if (rc != GM_OK) return rc;
  if (!batch || !batch->state) return fail(c, GM_E_ARG, "gm_sac_learner_grad_pi: incomplete batch (state)");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, sac_launch_grad_pi(l, batch->state, n, alpha, seed, draw, z, u, a, logp, q1, q2));
  HIPCHK(c, sac_launch_step(l, false, true, false, nullptr, 0.0f, n, nullptr));
  return GM_OK;
}

int gm_sac_learner_step_q(gm_sac_learner* l) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  l->step_q++;
  HIPCHK(c, sac_launch_step(l, true, false, true, nullptr, 0.0f, 1, nullptr));
  return GM_OK;
}

int gm_sac_learner_step_pi(gm_sac_learner* l) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  l->step_pi++;
  HIPCHK(c, sac_launch_step(l, false, false, true, nullptr, 0.0f, 1, nullptr));
  return GM_OK;
}

int gm_sac_soft_update(gm_sac* target, gm_sac* online, float tau) {
  if (!target || !target->ctx || !online) return GM_E_ARG;
  gm_ctx* c = target->ctx;
  if (online->ctx != c) return fail(c, GM_E_ARG, "gm_sac_soft_update: the two handles belong to different contexts");
  if (!sac_same_sizes(target, online)) return fail(c, GM_E_ARG, "gm_sac_soft_update: the two handles have different network sizes");
  if (!(tau >= 0.0f && tau <= 1.0f)) return fail(c, GM_E_ARG, "gm_sac_soft_update: tau in [0, 1] expected");
  HIPCHK(c, hipSetDevice(c->device));
  GlStepArgs a{};
  a.do_soft = 1;
  a.total = (long long)online->total;
  a.p = online->d_params;
  a.target = target->d_params;
  a.tau = tau;
  const int threads = 256;
  hipLaunchKernelGGL(gm_learn_step_kernel, dim3((unsigned)((a.total + threads - 1) / threads)), dim3(threads), 0,
                     c->stream, a);
  HIPCHK(c, hipGetLastError());
  return GM_OK;
}

int gm_sac_learner_read(gm_sac_learner* l, float* grad_flat, float* loss_q, float* loss_pi) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  if (grad_flat) {
    const int rc = sac_learner_unpack(c, l->online, l->d_grad, grad_flat);
    if (rc != GM_OK) return rc;
  }
  float both[2];
  const int rc = read_back(c, both, l->d_loss, sizeof(both));
  if (rc != GM_OK) return rc;
  if (loss_q) *loss_q = both[0];
  if (loss_pi) *loss_pi = both[1];
  return GM_OK;
}

int gm_sac_learner_get_state(gm_sac_learner* l, int64_t* steps, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  if (steps) { steps[0] = l->step_q; steps[1] = l->step_pi; }
  const float* src[3] = {l->d_m, l->d_v, l->d_vmax};
  float* dst[3] = {exp_avg, exp_avg_sq, max_exp_avg_sq};
  for (int i = 0; i < 3; i++)
    if (dst[i]) {
      const int rc = sac_learner_unpack(c, l->online, src[i], dst[i]);
      if (rc != GM_OK) return rc;
    }
  return GM_OK;
}

int gm_sac_learner_set_state(gm_sac_learner* l, const int64_t* steps, const float* exp_avg, const float* exp_avg_sq,
                             const float* max_exp_avg_sq) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  if (steps && (steps[0] < 0 || steps[1] < 0)) return fail(c, GM_E_ARG, "gm_sac_learner_set_state: negative step");
  HIPCHK(c, hipSetDevice(c->device));
  const float* src[3] = {exp_avg, exp_avg_sq, max_exp_avg_sq};
  float* dst[3] = {l->d_m, l->d_v, l->d_vmax};
  gm_sac* p = l->online;
  std::vector<float> packed((size_t)p->total);
  for (int i = 0; i < 3; i++)
    if (src[i]) {
      gsl_pack(p->net, p->total, src[i], packed.data());
      const int rc = stage_upload(c, dst[i], packed.data(), sizeof(float) * (size_t)p->total);
      if (rc != GM_OK) return rc;
    }
  if (steps) { l->step_q = steps[0]; l->step_pi = steps[1]; }
  return GM_OK;
}

int gm_sac_learner_train(gm_sac_learner* l, gm_sac* target, const gm_sac_replay* replay, int64_t size, int batch,
                         uint64_t seed, uint64_t noise_seed, uint64_t draw0, int n_updates, float gamma, float alpha,
                         int bootstrap_truncated, float tau, float* losses) {
  if (!l || !l->ctx) return GM_E_ARG;
  gm_ctx* c = l->ctx;
  gm_sac* online = l->online;
  if (!target) return fail(c, GM_E_ARG, "gm_sac_learner_train: no target handle");
  if (target->ctx != c) return fail(c, GM_E_ARG, "gm_sac_learner_train: the two handles belong to different contexts");
  if (!sac_same_sizes(target, online)) return fail(c, GM_E_ARG, "gm_sac_learner_train: the two handles have different network sizes");
  if (n_updates < 1) return fail(c, GM_E_ARG, "gm_sac_learner_train: n_updates < 1");
  if (batch > GL_MAX_BATCH)
    return fail(c, GM_E_ARG, "gm_sac_learner_train: batch " + std::to_string(batch) + ", the learner holds " +
                                 std::to_string(GL_MAX_BATCH));
  if (tau > 0.0f && (target == online || !(tau <= 1.0f)))
    return fail(c, GM_E_ARG, "gm_sac_learner_train: a polyak update needs a target handle of its own and tau <= 1");
  gm_sac* soft = tau > 0.0f ? target : nullptr;
  const gm_sac_batch b{l->d_state, l->d_action, l->d_next, l->d_reward, l->d_end, l->d_index};
  for (int u = 0; u < n_updates; u++) {
    const uint64_t d = draw0 + (uint64_t)u;
    int rc = gm_sac_replay_sample(c, replay, size, batch, seed, d, &b);   // (validates replay, size, batch)
    if (rc == GM_OK)
      rc = gm_sac_target(target, online, &b, batch, gamma, alpha, bootstrap_truncated, noise_seed, 2 * d, l->d_y, nullptr,
                         nullptr, nullptr, nullptr);
    if (rc != GM_OK) return rc;
    HIPCHK(c, sac_launch_grad_q(l, l->d_state, l->d_action, l->d_y, batch));
    l->step_q++;
    // (each range's polyak update rides in its step launch: elementwise what gm_sac_soft_update does after both steps)
    HIPCHK(c, sac_launch_step(l, true, true, true, soft, tau, batch, losses ? losses + 2 * u : nullptr));
    HIPCHK(c, sac_launch_grad_pi(l, l->d_state, batch, alpha, noise_seed, 2 * d + 1, nullptr, nullptr, nullptr, nullptr,
                                 nullptr, nullptr));
    l->step_pi++;
    HIPCHK(c, sac_launch_step(l, false, true, true, soft, tau, batch, losses ? losses + 2 * u + 1 : nullptr));
  }
  return GM_OK;
}

}  // extern "C"
