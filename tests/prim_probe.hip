// prim_probe.hip -- test-only translation unit (tests/prim_lib.py builds it with libgm's flags,
// tests/test_device_primitives.py drives it): probe kernels that call the device's numeric and
// lane primitives on their own and write what they return, plus host wrappers that allocate,
// copy, launch, synchronise and free.  Every wrapper returns the first hipError_t that was not
// hipSuccess (0 when all went well).  Not part of libgm.
#include "gm_arrow.h"
#include "gm_math.h"
#include "gm_policy_net.h"

// ------------------------------------------------------------ kernels
enum { OP_SQRT_N = 0, OP_RSQ_N, OP_RCP_N, OP_RCP_REFINED, OP_RCP_PIV, OP_GM_SIN, OP_GM_COS, OP_COUNT };

extern "C" __global__ void prim_unary_kernel(int op, const double* __restrict__ x, double* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double v = x[i];
  double r;
  switch (op) {
    case OP_SQRT_N: r = sqrt_n(v); break;
    case OP_RSQ_N: r = rsq_n(v); break;
    case OP_RCP_N: r = rcp_n(v); break;
    case OP_RCP_REFINED: r = rcp_refined(v); break;
    case OP_RCP_PIV: r = rcp_piv(v); break;
    case OP_GM_SIN: r = gm_sin(v); break;
    default: r = gm_cos(v); break;
  }
  out[i] = r;
}

extern "C" __global__ void prim_binary_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                              double* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = div_n(a[i], b[i]);
}

// One wave.  out[slot][64]: slots 0..3 row_shr by 1, 2, 4, 8; 4..7 row_shl by 1, 2, 4, 8;
// 8..23 row_bcast k = 0..15; 24..87 readlane_real l = 0..63; 88 gmf::row_totals; then, for every
// CL of GM_NSEG_LIST in its order, gmf::chain_forward<CL> and after those gmf::chain_backward<CL>,
// called on the lanes below 48 as the solves call them (the other lanes write their input back).
#define PRIM_SLOT_SHR 0
#define PRIM_SLOT_SHL 4
#define PRIM_SLOT_BCAST 8
#define PRIM_SLOT_READLANE 24
#define PRIM_SLOT_TOTALS 88
#define PRIM_SLOT_CHAINS 89
#define X(n) +1
constexpr int PRIM_N_CL = 0 GM_NSEG_LIST;
#undef X
constexpr int PRIM_N_SLOTS = PRIM_SLOT_CHAINS + 2 * PRIM_N_CL;

extern "C" __global__ void __launch_bounds__(NT) prim_lanes_kernel(const double* __restrict__ x,
                                                                   const double* __restrict__ L,
                                                                   double* __restrict__ out) {
  const int lane = threadIdx.x;   // (launched with NT threads, one block)
  const int p = lane & 15;
  const real v = x[lane];
  real Ll[16];
#pragma unroll
  for (int k = 0; k < 16; k++) Ll[k] = L[lane * 16 + k];
#pragma unroll
  for (int o = 0; o < 4; o++) {
    out[(PRIM_SLOT_SHR + o) * NT + lane] = row_shr(v, 1 << o);
    out[(PRIM_SLOT_SHL + o) * NT + lane] = row_shl(v, 1 << o);
  }
#pragma unroll
  for (int k = 0; k < 16; k++) out[(PRIM_SLOT_BCAST + k) * NT + lane] = row_bcast(v, k);
#pragma unroll
  for (int l = 0; l < NT; l++) out[(PRIM_SLOT_READLANE + l) * NT + lane] = readlane_real(v, l);
  out[PRIM_SLOT_TOTALS * NT + lane] = gmf::row_totals(v);
  int slot = PRIM_SLOT_CHAINS;
#define X(n) { real y = v; if (lane < 48) y = gmf::chain_forward<(n) + 2>(y, Ll, p); out[(slot++) * NT + lane] = y; }
  GM_NSEG_LIST
#undef X
#define X(n) { real y = v; if (lane < 48) y = gmf::chain_backward<(n) + 2>(y, Ll, p); out[(slot++) * NT + lane] = y; }
  GM_NSEG_LIST
#undef X
}

// One thread per case.  in[case][45]: a[3] b[3] M[9] qa[4] qb[4] ci[10] v[6] w[6].
// out[case][73]: the file-scope copy's dot3(a, b) cross3(a, b) mulmv3(M, a) mulmtv3(M, a)
// quat2mat(qa) quatmul(qa, qb) quatnorm(qa) (27 values), the gmf:: copy's same 27, then gmf::
// inert_mul(ci, v) cross_motion(v, w) cross_force(v, w) dot6(v, w) (19 values).
#define PRIM_HELPERS_IN 45
#define PRIM_HELPERS_OUT 73
extern "C" __global__ void prim_helpers_kernel(const double* __restrict__ in, double* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  real c[PRIM_HELPERS_IN];
  for (int k = 0; k < PRIM_HELPERS_IN; k++) c[k] = in[(size_t)i * PRIM_HELPERS_IN + k];
  const real *a = c, *b = c + 3, *M = c + 6, *qa = c + 15, *qb = c + 19, *ci = c + 23, *v = c + 33, *w = c + 39;
  real* o = out + (size_t)i * PRIM_HELPERS_OUT;
  real q[4];
  o[0] = dot3(a, b);
  cross3(o + 1, a, b);
  mulmv3(o + 4, M, a);
  mulmtv3(o + 7, M, a);
  quat2mat(o + 10, qa);
  quatmul(o + 19, qa, qb);
  ld4(q, qa);
  quatnorm(q);
  for (int k = 0; k < 4; k++) o[23 + k] = q[k];
  o += 27;
  o[0] = gmf::dot3(a, b);
  gmf::cross3(o + 1, a, b);
  gmf::mulmv3(o + 4, M, a);
  gmf::mulmtv3(o + 7, M, a);
  gmf::quat2mat(o + 10, qa);
  gmf::quatmul(o + 19, qa, qb);
  ld4(q, qa);
  gmf::quatnorm(q);
  for (int k = 0; k < 4; k++) o[23 + k] = q[k];
  o += 27;
  gmf::inert_mul(o, ci, v);
  gmf::cross_motion(o + 6, v, w);
  gmf::cross_force(o + 12, v, w);
  o[18] = gmf::dot6(v, w);
}

// Thread i: gp_choose on logits row i with global env id gid0 + i (softmax to q row i), then a
// second gp_softmax_argmax for the maximum (qbest[i]).
extern "C" __global__ void prim_choose_kernel(const float* __restrict__ logits, int n, int n_out, float eps,
                                              uint64_t seed, uint64_t decision, uint64_t gid0,
                                              int* __restrict__ actions, float* __restrict__ q,
                                              float* __restrict__ qbest) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* x = logits + (size_t)i * n_out;
  actions[i] = gp_choose(x, n_out, eps, seed, decision, gid0 + (uint64_t)i, q + (size_t)i * n_out);
  float qb;
  gp_softmax_argmax(x, n_out, nullptr, &qb);
  qbest[i] = qb;
}

extern "C" __global__ void prim_mix_kernel(const uint64_t* __restrict__ z, uint64_t* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = gp_mix(z[i]);
}

// ------------------------------------------------------------ host wrappers
namespace {
// device buffers of one call: freed on every way out
struct Bufs {
  void* p[8];
  int n = 0;
  hipError_t err = hipSuccess;
  void* alloc(size_t bytes) {
    void* d = nullptr;
    if (err != hipSuccess) return nullptr;
    err = hipMalloc(&d, bytes ? bytes : 1);
    if (err == hipSuccess) p[n++] = d;
    return d;
  }
  void* in(const void* h, size_t bytes) {
    void* d = alloc(bytes);
    if (err == hipSuccess && bytes) err = hipMemcpy(d, h, bytes, hipMemcpyHostToDevice);
    return d;
  }
  void out(void* h, const void* d, size_t bytes) {
    if (err == hipSuccess && bytes) err = hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost);
  }
  void launched() {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
  }
  ~Bufs() {
    for (int i = 0; i < n; i++) (void)hipFree(p[i]);
  }
};
int finish(Bufs& B) { return (int)B.err; }
constexpr int BLOCK = 256;
int blocks(int n) { return (n + BLOCK - 1) / BLOCK; }
}   // namespace

extern "C" {

int prim_op_count() { return OP_COUNT; }
int prim_n_slots() { return PRIM_N_SLOTS; }
int prim_helpers_in() { return PRIM_HELPERS_IN; }
int prim_helpers_out() { return PRIM_HELPERS_OUT; }
// the compiled chain lengths CL = n_seg + 2 in the order of the chain slots; returns their count
int prim_chain_lengths(int* cl) {
  int k = 0;
#define X(n) cl[k++] = (n) + 2;
  GM_NSEG_LIST
#undef X
  return k;
}
// 1 in the calibration build (-DGM_CAL_TU), else 0
int prim_is_cal() {
#ifdef GM_CAL_TU
  return 1;
#else
  return 0;
#endif
}

int prim_unary(int op, const double* x, double* out, int n) {
  if (op < 0 || op >= OP_COUNT || n < 1) return (int)hipErrorInvalidValue;
  Bufs B;
  const size_t bytes = (size_t)n * sizeof(double);
  const double* dx = (const double*)B.in(x, bytes);
  double* dout = (double*)B.alloc(bytes);
  if (B.err == hipSuccess) {
    hipLaunchKernelGGL(prim_unary_kernel, dim3(blocks(n)), dim3(BLOCK), 0, 0, op, dx, dout, n);
    B.launched();
  }
  B.out(out, dout, bytes);
  return finish(B);
}

int prim_binary(const double* a, const double* b, double* out, int n) {
  if (n < 1) return (int)hipErrorInvalidValue;
  Bufs B;
  const size_t bytes = (size_t)n * sizeof(double);
  const double* da = (const double*)B.in(a, bytes);
  const double* db = (const double*)B.in(b, bytes);
  double* dout = (double*)B.alloc(bytes);
  if (B.err == hipSuccess) {
    hipLaunchKernelGGL(prim_binary_kernel, dim3(blocks(n)), dim3(BLOCK), 0, 0, da, db, dout, n);
    B.launched();
  }
  B.out(out, dout, bytes);
  return finish(B);
}

// x[64], L[64][16], out[prim_n_slots()][64]
int prim_lanes(const double* x, const double* L, double* out) {
  Bufs B;
  const size_t obytes = (size_t)PRIM_N_SLOTS * NT * sizeof(double);
  const double* dx = (const double*)B.in(x, NT * sizeof(double));
  const double* dL = (const double*)B.in(L, NT * 16 * sizeof(double));
  double* dout = (double*)B.alloc(obytes);
  if (B.err == hipSuccess) {
    hipLaunchKernelGGL(prim_lanes_kernel, dim3(1), dim3(NT), 0, 0, dx, dL, dout);
    B.launched();
  }
  B.out(out, dout, obytes);
  return finish(B);
}

int prim_helpers(const double* in, double* out, int n) {
  if (n < 1) return (int)hipErrorInvalidValue;
  Bufs B;
  const size_t ibytes = (size_t)n * PRIM_HELPERS_IN * sizeof(double), obytes = (size_t)n * PRIM_HELPERS_OUT * sizeof(double);
  const double* din = (const double*)B.in(in, ibytes);
  double* dout = (double*)B.alloc(obytes);
  if (B.err == hipSuccess) {
    hipLaunchKernelGGL(prim_helpers_kernel, dim3(blocks(n)), dim3(BLOCK), 0, 0, din, dout, n);
    B.launched();
  }
  B.out(out, dout, obytes);
  return finish(B);
}

int prim_choose(const float* logits, int n, int n_out, float eps, uint64_t seed, uint64_t decision, uint64_t gid0,
                int* actions, float* q, float* qbest) {
  if (n < 1 || n_out < 1) return (int)hipErrorInvalidValue;
  Bufs B;
  const size_t lbytes = (size_t)n * n_out * sizeof(float);
  const float* dl = (const float*)B.in(logits, lbytes);
  int* da = (int*)B.alloc((size_t)n * sizeof(int));
  float* dq = (float*)B.alloc(lbytes);
  float* dqb = (float*)B.alloc((size_t)n * sizeof(float));
  if (B.err == hipSuccess) {
    hipLaunchKernelGGL(prim_choose_kernel, dim3(blocks(n)), dim3(BLOCK), 0, 0, dl, n, n_out, eps, seed, decision, gid0,
                       da, dq, dqb);
    B.launched();
  }
  B.out(actions, da, (size_t)n * sizeof(int));
  B.out(q, dq, lbytes);
  B.out(qbest, dqb, (size_t)n * sizeof(float));
  return finish(B);
}

int prim_mix(const uint64_t* z, uint64_t* out, int n) {
  if (n < 1) return (int)hipErrorInvalidValue;
  Bufs B;
  const size_t bytes = (size_t)n * sizeof(uint64_t);
  const uint64_t* dz = (const uint64_t*)B.in(z, bytes);
  uint64_t* dout = (uint64_t*)B.alloc(bytes);
  if (B.err == hipSuccess) {
    hipLaunchKernelGGL(prim_mix_kernel, dim3(blocks(n)), dim3(BLOCK), 0, 0, dz, dout, n);
    B.launched();
  }
  B.out(out, dout, bytes);
  return finish(B);
}

// the host build of the shared gm_sincos: needs no GPU
void host_sincos(const double* x, double* s, double* c, int n) {
  for (int i = 0; i < n; i++) gm_sincos(x[i], &s[i], &c[i]);
}

}   // extern "C"
