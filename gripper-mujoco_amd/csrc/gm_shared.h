// gm_shared.h -- shared by every stage of the env-step kernel: wave size and sync macros, the
// opaque lane id and the scheduling pins, the compiled chain lengths, `real`, DebugOut, the
// phase clock macros, and SharedT, the per-env LDS image (each stage header names the fields
// it reads and writes).  Restates no reference function.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gm_state.h"
#include "gm_math.h"

#define NT 64
// Phase boundary inside one env's physics.  Every kernel that runs the substep is launched
// with one 64-lane wavefront per workgroup (NT), and a wave's LDS operations complete in
// issue order, so a lane's read issued after another lane's write sees it: the boundary
// only has to stop the compiler moving LDS accesses across it.  __syncthreads' workgroup
// fence is lowered to an s_waitcnt lgkmcnt(0) drain at every boundary, stalling the wave
// on loads whose results it does not yet need.
#define GM_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); \
                            __builtin_amdgcn_wave_barrier(); } while (0)
// Synchronisation of the env's own work, which one wave does: __syncthreads' fences around
// a wave barrier instead of s_barrier.  For the 64-thread workgroups this is what
// __syncthreads lowers to anyway; in a DUO workgroup (gm_step_kernel<.., true>: a second,
// helper wave runs the collider concurrently, duo_helper) the helper is parked at its own
// s_barrier handshake and must not be counted by the owner wave's bookkeeping syncs.
#define GM_ENV_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); \
                           __builtin_amdgcn_wave_barrier(); \
                           __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); } while (0)
// The lane id, opaque to the compiler: each phase derives its lane predicates (chain row,
// border, contact lane, ...) from its own copy, so they are recomputed per phase instead of
// being computed once per substep and held live (in spilled SGPR pairs) across all of them.
__device__ __forceinline__ int fresh_lane() {
  int lane;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
  return lane;
}
// Pins a value's computation to the current block: the optimizer otherwise sinks the
// operands of a select or a conditional store (LDS loads, dot products) into a divergent
// branch per entry, each with its own load -> wait -> use chain.
__device__ __forceinline__ void keep(double x) { asm volatile("" ::"v"(x)); }
// ... and a batch of up to 13 values at once: their loads are all issued before the one
// wait (the scheduler otherwise issues each just before its use, one latency per entry)
template <int N>
__device__ __forceinline__ void keep_n(const double* a) {
  static_assert(N >= 1 && N <= 28, "keep_n: 1..28 values");
#define GM_K(i) "v"(a[(i) < N ? (i) : 0])
  if constexpr (N <= 13) {
    asm volatile("" ::GM_K(0), GM_K(1), GM_K(2), GM_K(3), GM_K(4), GM_K(5), GM_K(6), GM_K(7), GM_K(8), GM_K(9),
                 GM_K(10), GM_K(11), GM_K(12));
  } else {
    asm volatile("" ::GM_K(0), GM_K(1), GM_K(2), GM_K(3), GM_K(4), GM_K(5), GM_K(6), GM_K(7), GM_K(8), GM_K(9),
                 GM_K(10), GM_K(11), GM_K(12), GM_K(13), GM_K(14), GM_K(15), GM_K(16), GM_K(17), GM_K(18),
                 GM_K(19), GM_K(20), GM_K(21), GM_K(22), GM_K(23), GM_K(24), GM_K(25), GM_K(26), GM_K(27));
  }
#undef GM_K
}
#define GM_BB_SLOTS 18   // box-box hit slots in the LDS union (18 x 256 B; SharedT asserts it fits
                         // inside the union's CL-independent chain-root stage, so it never grows LDS)
// gm_step_kernel is instantiated per finger chain length (CL = n_seg + 2) so every chain
// recursion is unrolled into registers; GM_NSEG_LIST is the set compiled in.
#ifndef GM_NSEG_LIST
#define GM_NSEG_LIST X(5) X(6) X(7) X(8) X(9) X(10)
#endif
#define CLMAX (GM_MAX_SEG + 2)
#define TRI(p, q) ((p) * ((p) + 1) / 2 + (q))
#define TRIF ((CLMAX + 1) * (CLMAX + 2) / 2)
#define CW (CL + 8)   // compact row: obj[6], base, chain[CL] (+1 scratch slot); needs CL in scope
#define PI_F 3.14159265358979f
// lanes GM_OBJ_LANE0 .. + 5: the object's six dofs / velocity components, one per lane.  They
// lie past every scan lane (GmTopo::lane_body: finger f's links on lanes 16 f + 1 .. 16 f + CL,
// base, palm and object on GM_LANE_BASE .. + 2) and are not lane 0.
#define GM_LANE_BASE 48
#define GM_OBJ_LANE0 57
static_assert(32 + CLMAX < GM_LANE_BASE && GM_LANE_BASE + 2 < GM_OBJ_LANE0 && GM_OBJ_LANE0 + 6 <= 64,
              "the object's component lanes must hold no body's scan lane");

// `real` is the dynamics type: fp64, MuJoCo's mjtNum.  Kinematics, dynamics, collision
// geometry and the PGS solve all run in it (see DESIGN.md "Precision").
typedef double real;
// Env-step bookkeeping (sense / events / obs / done / reward) is inlined into the kernel;
// the substep loop is one outlined call per env-step (substep_loop).
#define GM_EPI_ATTR __device__

struct DebugOut {
  int32_t* ncon;      // [n_envs]
  double* contact;    // [n_envs][GM_MAX_CON][16]
  double* efc_force;  // [n_envs][GM_MAX_EFC]
  double* qacc;       // [n_envs][GM_MAX_DOF]
  unsigned long long* phase;   // [n_envs][GM_NPHASE] shader-clock cycles per phase (profiling)
  int32_t* nefc;      // [n_envs]
  double* wrench;     // [n_envs][6] the live object's cfrc_ext, [force; torque]
};
#define GM_NPHASE 32   // 0-27 shader clocks (see gmx.env PHASES), 28: sum of nefc, 29: substeps running MPR,
                       // 30: Newton iterations, 31: line-search evaluations

// Per-env LDS image, sized for the compile-time finger chain length CL = n_seg + 2:
// NB = 3 CL + 4 bodies (world, base, 3 x CL finger links, palm, object),
// NV = 3 CL + 8 dofs (base, 3 x CL, palm, free object).  gm_create checks the model.
template <int CL>
struct __align__(16) SharedT {
  static constexpr int NB = 3 * CL + 4;
  static constexpr int NV = 3 * CL + 8;
  static constexpr int TRIC = (CL + 1) * (CL + 2) / 2;
  GmEnvHot s;                     // the env's state minus its sensor windows
  real lock_pre[GM_MAX_LOCK];     // pre-integration qpos of the lock dofs (weld re-anchoring)
  real lrow_D[GM_MAX_LOCK + 1], lrow_aref[GM_MAX_LOCK + 1];   // lock rows (lock_rows; + a spare slot)
  int32_t lrow_dof[GM_MAX_LOCK + 2];
  real qacc[NV];                  // the Newton iterate; the substep's qacc at the end
  real xs[NV];                    // the Newton point x (line search: the step d = x - q)
  real Ma[NV], Mv[NV];            // H~ q and H~ d
  real xpos[NB][3];
  real xquat[NB][4];   // normalised body orientations; xmat = quat2mat(xquat)
  real Hf[3][TRIC], Hp[3], Ho[21], Hbb;   // H~ tree blocks (finger rows p = 0 base .. CL)
  real cdof[NV][6];
  real frc[NV];                   // smooth force: passive + PD actuation - bias
  real go[27];                    // the object's ground-contact K (21) and force (6)
  // contact record: dist, pos[3], normal[3], t1[3] (t2 = normal x t1), mu, force[3]
  // (contact frame, after the solve)
  real con[GM_MAX_CON][14];
  int16_t cgeom[GM_MAX_CON][2];   // canonical (geom1, geom2)
  int16_t cbody[GM_MAX_CON][2];   // their bodies
  int16_t pair_off[GM_MAX_PAIR], pair_cnt[GM_MAX_PAIR];   // contact slots of each candidate pair
  // LDS shared in time: the dynamics scratch is dead once H~ and the forces are formed; the
  // Newton stages then reuse it (body velocities + per-contact Q / F; the chain-root stage;
  // the factor's transfers; the debug copy of the row forces)
  union {
    struct {                  // kinematics .. mass matrix
      union {                 // composite inertia accumulates in place over cinert
        real cinert[NB][10];
        real Ic[NB][10];
      };
      real cfrc[NB][6];
      real chain_f[5][6], chain_I[5][10];   // chain-root sums for the base body
    };
    struct { real QF[GM_MAX_CON][9]; real V[NB][6]; } nw;
    struct { real V[NB][6]; real V2[NB][6]; } nw2;   // setup: qvel and warm-start velocities
    // the chain-root stage sits after the per-contact Q / F (the ground pass re-reads them)
    struct { real qf_[GM_MAX_CON][9]; real root[4][54]; real comp[54]; real oo[27]; } st;
    struct { real lbub[3][CL][14]; real plb[14]; real bbx[28]; real ych[3][CL]; real ypalm; } fs;
    struct { real efc[GM_MAX_EFC]; } dbg;
    // collision: the face-clipped box-box hits of pass 1 (point, depth), one slot of 8 per
    // face-case lane in lane order, for pass 2 to write without re-deriving the manifold
    struct { real hit[GM_BB_SLOTS][8][4]; } cl;
  };
  static_assert(sizeof(real[GM_BB_SLOTS][8][4]) <= sizeof(real) * (GM_MAX_CON * 9 + 4 * 54 + 54 + 27),
                "box-box hit slots must fit inside the chain-root stage (st): they may not grow the union");
  int32_t ncon, nefc, nl, overflow;
  int32_t res_valid;              // newton_solve: a capped solve's residual sits in Mv (euler_damping)
  int32_t duo_cmd;                // DUO workgroups: 1 = the helper wave runs this substep's collider, 0 = exit
  int32_t work_nefc, work_mpr, work_newton;   // this env-step's rows / MPR substeps / Newton iterations
  int32_t stp_fixed;              // update_all: `next` is a fixed point of the stepper this env-step (see there)
  float forces[32];            // extract_forces_faster results (see extract_forces)
  int32_t have_forces;
  float gauge_tmp[3];
  int32_t bend_ready;             // monitor_sensors: the bending gauges read this substep
  double next_read;               // substep_loop: sim time after which a sensor becomes ready
  unsigned long long tph[GM_NPHASE];
  GmEnvState* gs;                 // the env's record in HBM (sensor windows read / written there)
};

// per-phase shader-clock accounting (gm_step_profiled); needs `prof`, `lane`, `t0` in scope
#define PH(k) do { MARK(k); if (__builtin_expect(prof, 0)) { unsigned long long t_ = clock64(); if (lane == 0) S.tph[k] += t_ - t0; t0 = t_; } } while (0)
// developer marker for static per-phase instruction counts (GM_ISA_MARKERS builds: an
// s_nop 15 / s_nop k pair at every PH(k) in the disassembly)
#ifdef GM_ISA_MARKERS
#define MARK(k) asm volatile("s_nop 15\n\ts_nop " #k)
#else
#define MARK(k) do { } while (0)
#endif
