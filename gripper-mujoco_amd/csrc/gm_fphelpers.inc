// Floating-point helpers, included twice by gm_real.h: at file scope with FMA
// contraction off (everything the oracle must reproduce bit for bit: resets, spawns,
// stepper, sensors, observations) and inside namespace gmf with contraction on (the
// physics substep).  No include guard on purpose.

template <typename T> __device__ __forceinline__ T dot3(const T* a, const T* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
template <typename T> __device__ __forceinline__ void cross3(T* r, const T* a, const T* b) {
  T t0 = a[1] * b[2] - a[2] * b[1], t1 = a[2] * b[0] - a[0] * b[2], t2 = a[0] * b[1] - a[1] * b[0];
  r[0] = t0; r[1] = t1; r[2] = t2;
}
template <typename T> __device__ __forceinline__ void mulmv3(T* r, const T* M, const T* v) {
  T t0 = M[0] * v[0] + M[1] * v[1] + M[2] * v[2];
  T t1 = M[3] * v[0] + M[4] * v[1] + M[5] * v[2];
  T t2 = M[6] * v[0] + M[7] * v[1] + M[8] * v[2];
  r[0] = t0; r[1] = t1; r[2] = t2;
}
template <typename T> __device__ __forceinline__ void mulmtv3(T* r, const T* M, const T* v) {
  T t0 = M[0] * v[0] + M[3] * v[1] + M[6] * v[2];
  T t1 = M[1] * v[0] + M[4] * v[1] + M[7] * v[2];
  T t2 = M[2] * v[0] + M[5] * v[1] + M[8] * v[2];
  r[0] = t0; r[1] = t1; r[2] = t2;
}
template <typename T> __device__ __forceinline__ void quat2mat(T* R, const T* q) {
  T w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z);     R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y);     R[7] = 2 * (y * z + w * x);     R[8] = 1 - 2 * (x * x + y * y);
}
template <typename T> __device__ __forceinline__ void quatmul(T* r, const T* a, const T* b) {
  T t0 = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  T t1 = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  T t2 = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  T t3 = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  r[0] = t0; r[1] = t1; r[2] = t2; r[3] = t3;
}

__device__ __forceinline__ void quatnorm(real* q) {
  const real n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  real n = sqrt_n(n2);
  if (n < 1e-15) { q[0] = 1; q[1] = q[2] = q[3] = 0; return; }
#ifdef GM_FP_PHYSICS
  const real in = rsq_n(n2);   // (the physics copy: one refined reciprocal square root)
#else
  const real in = rcp_n(n);
#endif
  for (int i = 0; i < 4; i++) q[i] *= in;
}

// spatial inertia (I_O sym6, h = m c, m) times motion [w; v]
__device__ __forceinline__ void inert_mul(real* r, const real* ci, const real* v) {
  const real* w = v; const real* u = v + 3;
  real Iw0 = ci[0] * w[0] + ci[3] * w[1] + ci[4] * w[2];
  real Iw1 = ci[3] * w[0] + ci[1] * w[1] + ci[5] * w[2];
  real Iw2 = ci[4] * w[0] + ci[5] * w[1] + ci[2] * w[2];
  real hxu[3], hxw[3];
  cross3(hxu, ci + 6, u);
  cross3(hxw, ci + 6, w);
  r[0] = Iw0 + hxu[0]; r[1] = Iw1 + hxu[1]; r[2] = Iw2 + hxu[2];
  r[3] = ci[9] * u[0] - hxw[0]; r[4] = ci[9] * u[1] - hxw[1]; r[5] = ci[9] * u[2] - hxw[2];
}
__device__ __forceinline__ void cross_motion(real* r, const real* v, const real* mv) {
  real a[3], b[3], c[3];
  cross3(a, v, mv); cross3(b, v, mv + 3); cross3(c, v + 3, mv);
  r[0] = a[0]; r[1] = a[1]; r[2] = a[2];
  r[3] = b[0] + c[0]; r[4] = b[1] + c[1]; r[5] = b[2] + c[2];
}
__device__ __forceinline__ void cross_force(real* r, const real* v, const real* f) {
  real a[3], b[3], c[3];
  cross3(a, v, f); cross3(b, v + 3, f + 3); cross3(c, v, f + 3);
  r[0] = a[0] + b[0]; r[1] = a[1] + b[1]; r[2] = a[2] + b[2];
  r[3] = c[0]; r[4] = c[1]; r[5] = c[2];
}
__device__ __forceinline__ real dot6(const real* a, const real* b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3] + a[4] * b[4] + a[5] * b[5];
}

