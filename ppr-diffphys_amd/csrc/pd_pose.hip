// SE(3) pose algebra of the loss plumbing as single launches.
//
// The reference composes these from dqtorch's CUDA quaternion kernels and torch ops (diffphys/dp_utils.py:22-31
// compose_delta, :60-73 rotate_frame, :76-84 rotate_frame_vel; diffphys/geom_utils.py:148-203 se3_vec2mat / se3_mat2vec);
// the torch composition is ~200-450 launches forward and twice that backward per call on a few ten thousand poses:
// launch latency only.  Here every op is ONE launch forward and ONE launch for the vector-Jacobian product.
//
// The functions are written once, as templates over the scalar type.  The forward kernel instantiates them with float; the
// VJP kernel instantiates them with a dual number (value, one tangent) and sweeps the input directions -- forward-mode
// differentiation of exactly the code that produced the value, so the branch taken by the value (small-angle series, the
// best-conditioned quaternion candidate, clamps) is the branch that is differentiated, with torch's subgradient choices
// (d|a|/da = 0 at 0, sqrt_pos' = 0 at x <= 0, clamp' = 1 at the bound).  13-14 sweeps of ~150 flops per pose: nothing.
//
// Conventions (same as diffphys_amd/geom_utils.py): 7-vector = (p, q) with the quaternion's real part LAST; 6-vector =
// (p, axis-angle); matrices row-major; quaternion_to_matrix divides by |q|^2 (mocap quaternions arrive un-normalised).
#include <cstdio>
#include <hip/hip_runtime.h>
#include "../../include/ppr_diffphys.h"
#include "pd_device.h"  // PD_POSE_GROUND_WRENCH: the rollout kernels' own per-candidate contact code (contact_point_fwd / _adj / _adj_materials);
                        // PD_POSE_JOINT_COORDS: twist_angle, quat_decompose_cols / _adj and the quaternion adjoints;
                        // PD_POSE_JOINT_WRENCH: those, and joint_force / _adj, fixed_ang_h, clamp3_pass

// pd_host.hip: sets the text pd_last_error() returns, returns 1 (library-internal: hidden, no part of the C ABI)
__attribute__((visibility("hidden"))) int pd_set_error(const char *msg);

namespace {

struct Dual { float v, d; };
__device__ __forceinline__ Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Dual operator*(Dual a, Dual b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
__device__ __forceinline__ Dual operator/(Dual a, Dual b) { const float q = a.v / b.v; return {q, (a.d - q * b.d) / b.v}; }
__device__ __forceinline__ Dual operator+(float a, Dual b) { return {a + b.v, b.d}; }
__device__ __forceinline__ Dual operator-(float a, Dual b) { return {a - b.v, -b.d}; }
__device__ __forceinline__ Dual operator*(float a, Dual b) { return {a * b.v, a * b.d}; }
__device__ __forceinline__ Dual operator/(float a, Dual b) { const float q = a / b.v; return {q, -q * b.d / b.v}; }
__device__ __forceinline__ Dual operator*(Dual a, float b) { return {a.v * b, a.d * b}; }
__device__ __forceinline__ Dual operator/(Dual a, float b) { return {a.v / b, a.d / b}; }

__device__ __forceinline__ float val(float x) { return x; }
__device__ __forceinline__ float val(Dual x) { return x.v; }
__device__ __forceinline__ float t_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ Dual t_sqrt(Dual x) { const float s = sqrtf(x.v); return {s, 0.5f * x.d / s}; }
__device__ __forceinline__ float t_sin(float x) { return sinf(x); }
__device__ __forceinline__ Dual t_sin(Dual x) { return {sinf(x.v), cosf(x.v) * x.d}; }
__device__ __forceinline__ float t_cos(float x) { return cosf(x); }
__device__ __forceinline__ Dual t_cos(Dual x) { return {cosf(x.v), -sinf(x.v) * x.d}; }
__device__ __forceinline__ void set_const(float &x, float c) { x = c; }
__device__ __forceinline__ void set_const(Dual &x, float c) { x = {c, 0.0f}; }

// (r, i, j, k) real-FIRST -> 3x3 row-major   (geom_utils.quaternion_to_matrix)
template <class T>
__device__ __forceinline__ void quat_to_mat(T r, T i, T j, T k, T *R) {
  const T two_s = 2.0f / (r * r + i * i + j * j + k * k);
  R[0] = 1.0f - two_s * (j * j + k * k); R[1] = two_s * (i * j - k * r); R[2] = two_s * (i * k + j * r);
  R[3] = two_s * (i * j + k * r); R[4] = 1.0f - two_s * (i * i + k * k); R[5] = two_s * (j * k - i * r);
  R[6] = two_s * (i * k - j * r); R[7] = two_s * (j * k + i * r); R[8] = 1.0f - two_s * (i * i + j * j);
}

// axis-angle -> quaternion real-first   (geom_utils.axis_angle_to_quaternion: series below 1e-6 rad)
template <class T>
__device__ __forceinline__ void aa_to_quat(const T *a, T *q) {
  const T n2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
  T ang;
  if (val(n2) > 0.0f) ang = t_sqrt(n2); else set_const(ang, 0.0f);  // torch.norm: zero subgradient at 0
  const T half = 0.5f * ang;
  T s;
  if (fabsf(val(ang)) < 1e-6f) s = 0.5f - ang * ang / 48.0f; else s = t_sin(half) / ang;
  q[0] = t_cos(half); q[1] = a[0] * s; q[2] = a[1] * s; q[3] = a[2] * s;
}

// 3x3 row-major -> quaternion real-first, the best-conditioned of the four candidate forms   (geom_utils.matrix_to_quaternion)
template <class T>
__device__ __forceinline__ void mat_to_quat(const T *m, T *q) {
  const T x[4] = {1.0f + m[0] + m[4] + m[8], 1.0f + m[0] - m[4] - m[8], 1.0f - m[0] + m[4] - m[8], 1.0f - m[0] - m[4] + m[8]};
  T qa[4];
  int best = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (val(x[k]) > 0.0f) qa[k] = t_sqrt(x[k]); else set_const(qa[k], 0.0f);  // _sqrt_pos
    if (k > 0 && val(qa[k]) > val(qa[best])) best = k;                        // argmax: first maximum
  }
  const T a = m[7] - m[5], b = m[2] - m[6], c = m[3] - m[1], d = m[3] + m[1], e = m[2] + m[6], f = m[5] + m[7];
  T cand[4], den = qa[best];
  if (best == 0) { cand[0] = qa[0] * qa[0]; cand[1] = a; cand[2] = b; cand[3] = c; }
  else if (best == 1) { cand[0] = a; cand[1] = qa[1] * qa[1]; cand[2] = d; cand[3] = e; }
  else if (best == 2) { cand[0] = b; cand[1] = d; cand[2] = qa[2] * qa[2]; cand[3] = f; }
  else { cand[0] = c; cand[1] = e; cand[2] = f; cand[3] = qa[3] * qa[3]; }
  if (!(val(den) >= 0.1f)) set_const(den, 0.1f);  // clamp(min=0.1)
  den = 2.0f * den;
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = cand[k] / den;
}

// (p, q real-last) 7-vector -> R, p
template <class T>
__device__ __forceinline__ void pose7(const T *v, T *R, T *p) {
  quat_to_mat(v[6], v[3], v[4], v[5], R);
  p[0] = v[0]; p[1] = v[1]; p[2] = v[2];
}

// T = T_a @ T_b as the 4x4 product computes it, then se3_mat2vec(outdim 7)
template <class T>
__device__ __forceinline__ void compose_out7(const T *Ra, const T *pa, const T *Rb, const T *pb, T *out) {
  T R[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = Ra[3 * i] * Rb[j] + Ra[3 * i + 1] * Rb[3 + j] + Ra[3 * i + 2] * Rb[6 + j];
    out[i] = Ra[3 * i] * pb[0] + Ra[3 * i + 1] * pb[1] + Ra[3 * i + 2] * pb[2] + pa[i];
  }
  T q[4];
  mat_to_quat(R, q);
  out[3] = q[1]; out[4] = q[2]; out[5] = q[3]; out[6] = q[0];
}

enum { OP_COMPOSE_DELTA = PD_POSE_COMPOSE_DELTA, OP_ROTATE_FRAME = PD_POSE_ROTATE_FRAME, OP_ROTATE_VEL = PD_POSE_ROTATE_VEL,
       OP_PROJECT = PD_POSE_PROJECT, OP_PROJECT_POINT = PD_POSE_PROJECT_POINT };  // (PD_POSE_GROUND_WRENCH and PD_POSE_JOINT_COORDS have kernels of their own, below)

template <int OP> struct Shape;
template <> struct Shape<OP_COMPOSE_DELTA> { static constexpr int NA = 7, NB = 6, NO = 7; };  // a = target pose, b = delta (p, axis-angle)
template <> struct Shape<OP_ROTATE_FRAME> { static constexpr int NA = 7, NB = 7, NO = 7; };   // a = global pose, b = target pose
template <> struct Shape<OP_ROTATE_VEL> { static constexpr int NA = 7, NB = 6, NO = 6; };     // a = global pose, b = (linear, angular)
template <> struct Shape<OP_PROJECT> { static constexpr int NA = 16, NB = 7, NO = 2; };       // a = camera (rtk 4x4), b = pose (p used)
template <> struct Shape<OP_PROJECT_POINT> { static constexpr int NA = 16, NB = 10, NO = 2; };  // a = camera, b = (pose, body-frame point)

// Where element i finds its row of `a`.  Ops 0-2: a_sel is the row stride in floats (0 = ONE row shared by all).  Projection ops: a_sel is
// the group size g -- camera row i / g serves element i (0 = a row per element).
template <int OP>
__device__ __forceinline__ size_t a_offset(int i, int a_sel) {
  if (OP == OP_PROJECT || OP == OP_PROJECT_POINT) return (size_t)(a_sel ? i / a_sel : i) * Shape<OP>::NA;
  return (size_t)i * a_sel;
}

template <int OP, class T>
__device__ __forceinline__ void pose_fn(const T *a, const T *b, T *out) {
  if (OP == OP_COMPOSE_DELTA) {  // se3_mat2vec(se3_vec2mat(delta) @ se3_vec2mat(target))   dp_utils.py:22-31
    T q[4], R1[9], R2[9], p2[3];
    aa_to_quat(b + 3, q);
    quat_to_mat(q[0], q[1], q[2], q[3], R1);
    pose7(a, R2, p2);
    compose_out7(R1, b, R2, p2, out);
  } else if (OP == OP_ROTATE_FRAME) {  // se3_mat2vec(se3_vec2mat(global) @ se3_vec2mat(target))   dp_utils.py:60-73
    T Rg[9], pg[3], R2[9], p2[3];
    pose7(a, Rg, pg);
    pose7(b, R2, p2);
    compose_out7(Rg, pg, R2, p2, out);
  } else if (OP == OP_PROJECT || OP == OP_PROJECT_POINT) {  // project_bodies   dp_utils.py:200-214
    // a = rtk: rows 0-2 [R|t] world -> view, row 3 (fx, fy, cx, cy); K @ (R p + t), then the division by its third entry -- no clamp
    T p[3] = {b[0], b[1], b[2]};
    if (OP == OP_PROJECT_POINT) {  // the body-frame point b[7..9] instead of the body origin: p + R(q) c
      T Rb[9];
      quat_to_mat(b[6], b[3], b[4], b[5], Rb);
#pragma unroll
      for (int i = 0; i < 3; ++i) p[i] = p[i] + (Rb[3 * i] * b[7] + Rb[3 * i + 1] * b[8] + Rb[3 * i + 2] * b[9]);
    }
    T v[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = a[4 * i] * p[0] + a[4 * i + 1] * p[1] + a[4 * i + 2] * p[2] + a[4 * i + 3];
    out[0] = (a[12] * v[0] + a[14] * v[2]) / v[2];
    out[1] = (a[13] * v[1] + a[15] * v[2]) / v[2];
  } else {  // both halves rotated by the rotation of global   dp_utils.py:76-84
    T Rg[9];
    quat_to_mat(a[6], a[3], a[4], a[5], Rg);
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 3; ++i) out[3 * h + i] = Rg[3 * i] * b[3 * h] + Rg[3 * i + 1] * b[3 * h + 1] + Rg[3 * i + 2] * b[3 * h + 2];
  }
}

template <int OP>
__global__ __launch_bounds__(256) void k_pose_fwd(int n, const float *__restrict__ a, int a_sel, const float *__restrict__ b,
                                                  float *__restrict__ out) {
  using S = Shape<OP>;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float av[S::NA], bv[S::NB], o[S::NO];
#pragma unroll
  for (int k = 0; k < S::NA; ++k) av[k] = a[a_offset<OP>(i, a_sel) + k];
#pragma unroll
  for (int k = 0; k < S::NB; ++k) bv[k] = b[(size_t)i * S::NB + k];
  pose_fn<OP, float>(av, bv, o);
#pragma unroll
  for (int k = 0; k < S::NO; ++k) out[(size_t)i * S::NO + k] = o[k];
}

template <int OP>
__global__ __launch_bounds__(256) void k_pose_vjp(int n, const float *__restrict__ a, int a_sel, const float *__restrict__ b,
                                                  const float *__restrict__ g_out, float *__restrict__ g_a, float *__restrict__ g_b) {
  using S = Shape<OP>;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Dual av[S::NA], bv[S::NB], o[S::NO];
  float g[S::NO];
#pragma unroll
  for (int k = 0; k < S::NA; ++k) av[k] = {a[a_offset<OP>(i, a_sel) + k], 0.0f};
#pragma unroll
  for (int k = 0; k < S::NB; ++k) bv[k] = {b[(size_t)i * S::NB + k], 0.0f};
#pragma unroll
  for (int k = 0; k < S::NO; ++k) g[k] = g_out[(size_t)i * S::NO + k];
  for (int dir = 0; dir < S::NA + S::NB; ++dir) {  // not unrolled: one copy of the function body
    const bool in_a = dir < S::NA;
    if (in_a ? g_a == nullptr : g_b == nullptr) continue;
#pragma unroll
    for (int k = 0; k < S::NA; ++k) av[k].d = (in_a && k == dir) ? 1.0f : 0.0f;
#pragma unroll
    for (int k = 0; k < S::NB; ++k) bv[k].d = (!in_a && k == dir - S::NA) ? 1.0f : 0.0f;
    pose_fn<OP, Dual>(av, bv, o);
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < S::NO; ++k) s += g[k] * o[k].d;
    if (in_a) g_a[(size_t)i * S::NA + dir] = s; else g_b[(size_t)i * S::NB + (dir - S::NA)] = s;
  }
}

// Lowest ground-contact candidate of each pose set: min over candidates c of  p_y[body(c)] + (R(q[body(c)]) point_c)_y - dist_c.
// One workgroup per pose set; ties go to the lowest candidate index; a NaN height wins (propagates like torch.min).
__global__ __launch_bounds__(256) void k_foot_height(int nb, int nc, const float *__restrict__ body_q, const int *__restrict__ c_body,
                                                     const float *__restrict__ c_point, const float *__restrict__ c_dist,
                                                     float *__restrict__ h_out, int *__restrict__ arg_out) {
  __shared__ float s_h[256];
  __shared__ int s_i[256];
  const float *X = body_q + (size_t)blockIdx.x * nb * 7;
  float best = INFINITY;
  int best_i = 0x7fffffff;
  bool best_nan = false;
  for (int c = threadIdx.x; c < nc; c += 256) {
    const float *x = X + (size_t)c_body[c] * 7;
    const float qx = x[3], qy = x[4], qz = x[5], w = x[6];
    const float px = c_point[3 * c], py = c_point[3 * c + 1], pz = c_point[3 * c + 2];
    const float rot_y = py * (2.0f * w * w - 1.0f) + 2.0f * w * (qz * px - qx * pz) + 2.0f * qy * (qx * px + qy * py + qz * pz);
    const float h = x[1] + rot_y - c_dist[c];
    const bool is_nan = h != h;
    if (!best_nan && (is_nan || h < best)) { best = h; best_i = c; best_nan = is_nan; }
  }
  s_h[threadIdx.x] = best; s_i[threadIdx.x] = best_i;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      const float h0 = s_h[threadIdx.x], h1 = s_h[threadIdx.x + off];
      const int i0 = s_i[threadIdx.x], i1 = s_i[threadIdx.x + off];
      const bool n0 = h0 != h0, n1 = h1 != h1;
      const bool take1 = n0 || n1 ? (n1 && (!n0 || i1 < i0)) : (h1 < h0 || (h1 == h0 && i1 < i0));
      if (take1) { s_h[threadIdx.x] = h1; s_i[threadIdx.x] = i1; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { h_out[blockIdx.x] = s_h[0]; arg_out[blockIdx.x] = s_i[0]; }
}

// d height / d body_q: non-zero for the body of the arg-min candidate only (the gradient torch.min routes to its index)
__global__ __launch_bounds__(256) void k_foot_height_vjp(int n, int nb, const float *__restrict__ body_q, const int *__restrict__ c_body,
                                                         const float *__restrict__ c_point, const int *__restrict__ arg,
                                                         const float *__restrict__ g_h, float *__restrict__ g_body_q) {
  const int i = blockIdx.x * 256 + threadIdx.x;  // (pose set, body)
  if (i >= n * nb) return;
  const int set = i / nb, body = i - set * nb, c = arg[set];
  float o[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c >= 0 && c_body[c] == body) {
    const float *x = body_q + (size_t)i * 7;
    const float qx = x[3], qy = x[4], qz = x[5], w = x[6], g = g_h[set];
    const float px = c_point[3 * c], py = c_point[3 * c + 1], pz = c_point[3 * c + 2];
    o[1] = g;
    o[3] = g * (-2.0f * w * pz + 2.0f * qy * px);
    o[4] = g * (2.0f * (qx * px + qy * py + qz * pz) + 2.0f * qy * py);
    o[5] = g * (2.0f * w * px + 2.0f * qy * pz);
    o[6] = g * (4.0f * w * py + 2.0f * (qz * px - qx * pz));
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) g_body_q[(size_t)i * 7 + k] = o[k];
}

// ---- PD_POSE_GROUND_WRENCH: the ground-contact contribution to body_f, G(state, materials) = -sum_c (r_c x f_c, f_c) over the body's
// touching candidates (integrator_euler.py:93-179), and its vector-Jacobian products.  The contact wrench of a step is a function of that
// step's state and of the materials alone (semi-implicit Euler) and enters body_f additively, so this one op, fully parallel over saved
// states, gives d loss / d materials = sum_t <g_res_f[t], dG/dmaterials> and a differentiable grf = res_f + G without touching a rollout
// kernel.  Per candidate it runs pd_device.h's contact_point_* on a record and cull vector staged as the forward kernels stage them
// (stage_record; rc and the cull vector through rotm): the rollout's values and its touch decision, candidate by candidate.
// Mapping: one wavefront per element (= body of a state set), four per workgroup; lanes stride over the body's candidates, per-lane
// partial sums, then a fixed-order xor butterfly across the wave.  No atomics, no LDS, no barrier: the same bits on every run.
// Contact table: include/ppr_diffphys.h (hip_backend.contact_table builds it).
enum { GW_HEAD = 4, GW_BODY = 12 };
struct GwTable { int nmat; const float4 *mats, *pts; const float *body, *pmat; };
__device__ __forceinline__ GwTable gw_table(const float *t) {
  GwTable T;
  const int nb = (int)t[0], nc = (int)t[1];
  T.nmat = (int)t[2];
  T.mats = (const float4 *)(t + GW_HEAD);
  T.body = t + GW_HEAD + 4 * T.nmat;
  T.pts = (const float4 *)(T.body + GW_BODY * nb);
  T.pmat = (const float *)(T.pts + nc);
  return T;
}
__device__ __forceinline__ float wave_sum(float x) {  // every lane ends with the same sum, formed in the same order
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}
// Stages element i: the 17-float record and the cull vector of its state row, the candidate range of its body.  Returns false when no
// candidate can touch: the body has none, or its bounding sphere (centre, radius, largest dist; in the table) is provably above y = 0 --
// the lowest height over the sphere, p_y + row1 . centre - |row1| radius - max dist, beyond a slack 1 000 times the rounding of its
// terms.  A NaN / inf state fails the comparison and is swept.
__device__ __forceinline__ bool gw_stage(const GwTable &T, int body, const float *x, float *rec, float4 &cv, int &first, int &count, int &umat) {
  const float *B = T.body + GW_BODY * body;
  const BodyState s = load_state0(x, 0);
  float Rm[9];
  rotm(s.r, Rm);
  cv = stage_record(rec, &cv, 0, s, mat_vec(Rm, ld3(B)), Rm);
  first = (int)B[3]; count = (int)B[4]; umat = (int)B[11];  // umat: the one material of all the body's candidates, or -1 (mixed)
  if (count <= 0) return false;
  const float len = sqrtf(cv.y * cv.y + cv.z * cv.z + cv.w * cv.w);
  const float ylow = cv.x + (cv.y * B[5] + cv.z * B[6] + cv.w * B[7]) - 1.001f * len * B[8] - B[9];
  return !(ylow > 1e-4f * (1.0f + fabsf(cv.x) + len * B[10] + fabsf(B[9])));
}

__global__ __launch_bounds__(256) void k_ground_wrench_fwd(int n, int nb, const float *__restrict__ tab, const float *__restrict__ state,
                                                           float *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const GwTable T = gw_table(tab);
  float rec[PD_REC];
  float4 cv;
  int first, count, umat;
  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (gw_stage(T, (int)(i % nb), state + (size_t)i * PD_ADJ, rec, cv, first, count, umat)) {
    for (int k = lane; k < count; k += 64) {
      const int c = first + k;
      ContactOut o;
      if (contact_point_fwd(rec, cv, T.pts[c], T.mats[(int)T.pmat[c]], o)) {  // body_f -= (t, f)   (:179)
        acc[0] -= o.t.x; acc[1] -= o.t.y; acc[2] -= o.t.z; acc[3] -= o.f.x; acc[4] -= o.f.y; acc[5] -= o.f.z;
      }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) acc[j] = wave_sum(acc[j]);
  }
  if (lane < 6) {
    float v = acc[0];
#pragma unroll
    for (int j = 1; j < 6; ++j) v = lane == j ? acc[j] : v;
    out[(size_t)i * 6 + lane] = v;
  }
}

// g_b [n][13]: the raw partials of <g_out, G> with respect to the state row (quaternion entries not projected); g_a [n][nmat][4]: with
// respect to the material rows, per element.  Either may be NULL.  The two are separate sweeps, so the bits of one do not depend on
// whether the other was asked for; a body may mix materials: one masked sweep and one reduction per material row (a body of one material,
// which the table names, sweeps once).
__global__ __launch_bounds__(256) void k_ground_wrench_vjp(int n, int nb, const float *__restrict__ tab, const float *__restrict__ state,
                                                           const float *__restrict__ g_out, float *__restrict__ g_a, float *__restrict__ g_b) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const GwTable T = gw_table(tab);
  float rec[PD_REC];
  float4 cv;
  int first, count, umat;
  const bool sweep = gw_stage(T, (int)(i % nb), state + (size_t)i * PD_ADJ, rec, cv, first, count, umat);
  const v3 g_t = ld3(g_out + (size_t)i * 6), g_f = ld3(g_out + (size_t)i * 6 + 3);
  if (g_b) {
    float acc[PD_ADJ];
#pragma unroll
    for (int j = 0; j < PD_ADJ; ++j) acc[j] = 0.f;
    if (sweep) {
      // The state row is taken as it is, so its quaternion need not be unit -- and then qrot_inv(q, rc), from which contact_point_adj
      // recovers the body-frame centre of mass (the rollouts' states are normalised every step), is not com: the two-piece form with
      // the table's own com instead, so that g_b is the gradient of what the forward kernel computes for ANY row.
      const v3 com = ld3(T.body + GW_BODY * (int)(i % nb));
      for (int k = lane; k < count; k += 64) {
        const int c = first + k;
        const float4 P = T.pts[c], M = T.mats[(int)T.pmat[c]];
        ContactPre pre = contact_point_adj_pre(rec, cv, P, M);
        pre.com = com;
        BodyAdj o;
        if (contact_point_adj_rest(pre, P, M, g_t, g_f, o)) {
          float t[PD_ADJ];
          adj_store(t, o);
#pragma unroll
          for (int j = 0; j < PD_ADJ; ++j) acc[j] += t[j];
        }
      }
#pragma unroll
      for (int j = 0; j < PD_ADJ; ++j) acc[j] = wave_sum(acc[j]);
    }
    if (lane < PD_ADJ) {
      float v = acc[0];
#pragma unroll
      for (int j = 1; j < PD_ADJ; ++j) v = lane == j ? acc[j] : v;
      g_b[(size_t)i * PD_ADJ + lane] = v;
    }
  }
  if (g_a) {
    float *ga = g_a + (size_t)i * T.nmat * 4;
    if (!sweep) {
      for (int j = lane; j < T.nmat * 4; j += 64) ga[j] = 0.f;
      return;
    }
    for (int m = 0; m < T.nmat; ++m) {
      if (umat >= 0 && m != umat) {  // a body of ONE material (the usual case): the other rows are zero without a sweep
        if (lane < 4) ga[4 * m + lane] = 0.f;
        continue;
      }
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      for (int k = lane; k < count; k += 64) {
        const int c = first + k;
        float4 am;
        if ((int)T.pmat[c] == m && contact_point_adj_materials(rec, cv, T.pts[c], T.mats[m], g_t, g_f, am)) {
          a0 += am.x; a1 += am.y; a2 += am.z; a3 += am.w;
        }
      }
      a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2); a3 = wave_sum(a3);
      if (lane < 4) ga[4 * m + lane] = lane == 0 ? a0 : lane == 1 ? a1 : lane == 2 ? a2 : a3;
    }
  }
}

// ---- PD_POSE_JOINT_COORDS: joint coordinates (joint_q, joint_qd) of body states, the inverse of k_fk (Warp's eval_ik), and its
// vector-Jacobian product.  For body i with parent par the joint frame is X_wj = X_par X_p[i] (X_p[i] alone, w_p = v_p = 0, without a
// parent); r_err = conj(q_wj) q_c and w_err = w_c - w_p are the joint pass's (joint_ctx, pd_device.h; integrator_euler.py:326-372).
//   FREE      q = (R_wj^-1 (p_c - p_wj), r_err), qd = (R_wj^-1 w_err, R_wj^-1 (v_c - v_p - w_err x com)): fk_joint solved for its inputs
//   REVOLUTE  q = twist_angle (pd_math.h: :394-400 through atan2), qd = w_err . R_wj axis   -- what joint_fwd measures
//   COMPOUND  q = quat_decompose(conj(q_off) r_err q_off); measured rates m_k = (R_wj R_off a_k) . w_err on the axis chain of :418-427 --
//             what joint_fwd measures.  Rate mode 0 (measured): qd = m.  The a_k are not orthogonal (a_0 . a_1 = a_1 . a_2 = 0,
//             a_0 . a_2 = s = a_2.x), so m is not the generalised velocity of fk_joint_local's w_jc = sum a_k qd_k; rate mode 1
//             (generalized) solves the Gram system: qd_1 = m_1, (qd_0, qd_2) = ((m_0 - s m_2), (m_2 - s m_0)) / (1 - s^2) -- singular at
//             |q_1| = pi / 2 (gimbal lock), where the result is inf / NaN like any division by zero here.
//   FIXED     no coordinates
// Default numeric policy only: this translation unit is compiled once, with PD_POLICY 0; the literal-acos policy is not offered.
// Forward: one lane per element (= body of a state set); it reads its own row and its parent's, nothing is chained.
// VJP: a body's coordinates depend on its own row and on its parent's, so a parent receives up to JC_MAXCH contributions.  Whole state
// sets share a workgroup (256 / nb sets of nb lanes); every lane leaves the parent-side adjoint of its joint in an LDS slot and, after ONE
// barrier, adds its children's slots to its own-side adjoint in the table's child order (a parent gathers its
// children's in fixed order).  No atomics: the same bits on every run.  Joint table: include/ppr_diffphys.h (hip_backend.joint_table).
enum { JC_HEAD = 4, JC_BODY = 24, JC_MAXCH = 8, JC_MAXNB = 256 };
// Whole state sets per workgroup, a lane per body (k_joint_coords_vjp and the two centroidal kernels; nb <= 256): lane -> the set's index
// in the workgroup and in the launch, the body inside the set.  in_set: the lane belongs to one of the 256 / nb sets the workgroup
// places (the lanes past them idle); active: that set exists.
struct SetLane { int set_l, body; long long set; bool in_set, active; };
__device__ __forceinline__ SetLane set_lane(int nsets, int nb) {
  SetLane L;
  const int per_wg = 256 / nb;
  L.set_l = (int)threadIdx.x / nb; L.body = (int)threadIdx.x - L.set_l * nb;
  L.set = (long long)blockIdx.x * per_wg + L.set_l;
  L.in_set = L.set_l < per_wg; L.active = L.in_set && L.set < nsets;
  return L;
}
struct JcJoint {  // what the forward pass and the adjoint share
  int type, parent, qs, qds;
  v3 p_pj, axis, com;
  qt q_pj, q_off;
  v3 pp, w_p, v_p, p_wj, w_err;
  qt qp, q_wj, r_err;
};
// A table the call was not sized for must not send a lane out of bounds (the host cannot validate a device buffer): a parent index
// outside the set reads no row, and a joint whose coordinates do not lie inside [0, nq) x [0, nqd) -- or any joint of a table built for
// another nb -- is taken as FIXED: nothing of it is read or written.
// STRIDE: floats per row of set_rows (PD_ADJ: bare state rows; the joint wrench's rows carry the joint's controls behind the state).
template <int STRIDE>
__device__ __forceinline__ BodyState load_row(const float *rows, size_t i) {
  if constexpr (STRIDE == PD_ADJ) return load_state0(rows, i);
  const float *r = rows + i * STRIDE;
  BodyState s;
  s.p = ld3(r); s.r = ld4(r + 3); s.w = ld3(r + 7); s.v = ld3(r + 10);
  return s;
}
template <int STRIDE = PD_ADJ>
__device__ __forceinline__ JcJoint jc_joint(const float *tab, int nb, int nq, int nqd, int body, const BodyState &s, const float *set_rows) {
  JcJoint J;
  J.pp = V3(0, 0, 0); J.w_p = J.pp; J.v_p = J.pp; J.qp = Q4(0, 0, 0, 1);
  if ((int)tab[0] != nb) {  // not this call's table: no row of it is read
    J.parent = -1; J.type = PD_JOINT_FIXED; J.qs = J.qds = 0;
    J.p_pj = J.pp; J.axis = J.pp; J.com = J.pp; J.q_pj = J.qp; J.q_off = J.qp;
    J.p_wj = J.pp; J.q_wj = J.qp; J.r_err = s.r; J.w_err = s.w;
    return J;
  }
  const float *B = tab + JC_HEAD + JC_BODY * body;
  J.parent = (int)B[0]; J.type = (int)B[1]; J.qs = (int)B[2]; J.qds = (int)B[3];
  J.p_pj = ld3(B + 4); J.q_pj = ld4(B + 7); J.axis = ld3(B + 11); J.q_off = ld4(B + 14); J.com = ld3(B + 18);
  J.p_wj = J.p_pj; J.q_wj = J.q_pj;
  const int wq = J.type == PD_JOINT_FREE ? 7 : J.type == PD_JOINT_COMPOUND ? 3 : 1, wqd = wq == 7 ? 6 : wq;
  if (J.qs < 0 || J.qs + wq > nq || J.qds < 0 || J.qds + wqd > nqd) J.type = PD_JOINT_FIXED;
  if (J.parent >= nb) J.parent = -1;
  if (J.parent >= 0) {
    const BodyState P = load_row<STRIDE>(set_rows, (size_t)J.parent);
    J.pp = P.p; J.qp = P.r; J.w_p = P.w; J.v_p = P.v;
    J.p_wj = P.p + qrot(P.r, J.p_pj);
    J.q_wj = qmul(P.r, J.q_pj);
  }
  J.r_err = qmul(qconj(J.q_wj), s.r);
  J.w_err = s.w - J.w_p;
  return J;
}
struct JcCompound {  // the compound joint's forward pass, kept for its adjoint
  qt qa, q_pc, q_0, q_1, q10, q_w;
  v3 c0, c1, c2, a1, a2, u;
  float ang[3], m[3], qd[3], s, id;
};
__device__ __forceinline__ void jc_compound(const JcJoint &J, bool generalized, JcCompound &C) {
  C.qa = qmul(qconj(J.q_off), J.r_err);
  C.q_pc = qmul(C.qa, J.q_off);
  quat_decompose_cols(C.q_pc, C.ang, C.c0, C.c1, C.c2);
  C.q_0 = q_axis_angle(V3(1, 0, 0), C.ang[0]);  // the axis chain of integrator_euler.py:418-427
  C.a1 = qrot(C.q_0, V3(0, 1, 0));
  C.q_1 = q_axis_angle(C.a1, C.ang[1]);
  C.q10 = qmul(C.q_1, C.q_0);
  C.a2 = qrot(C.q10, V3(0, 0, 1));
  C.q_w = qmul(J.q_wj, J.q_off);
  C.u = qrot_inv(C.q_w, J.w_err);  // (R a) . w = a . (R^T w) for the linear map of ANY quaternion (pd_math.h rotm): m_k = a_k . u
  C.m[0] = C.u.x; C.m[1] = dot(C.a1, C.u); C.m[2] = dot(C.a2, C.u);
  C.s = C.a2.x; C.id = 1.0f;
  C.qd[0] = C.m[0]; C.qd[1] = C.m[1]; C.qd[2] = C.m[2];
  if (generalized) {
    C.id = 1.0f / (1.0f - C.s * C.s);
    C.qd[0] = (C.m[0] - C.s * C.m[2]) * C.id;
    C.qd[2] = (C.m[2] - C.s * C.m[0]) * C.id;
  }
}

__global__ __launch_bounds__(256) void k_joint_coords_fwd(int n, int nb, const float *__restrict__ tab, const float *__restrict__ state,
                                                          float *__restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int set = (int)(i / nb), body = (int)(i - (long long)set * nb);
  const int nq = (int)tab[1], nqd = (int)tab[2];
  const bool generalized = tab[3] != 0.0f;
  const float *rows = state + (size_t)set * nb * PD_ADJ;
  const BodyState s = load_state0(rows, (size_t)body);
  const JcJoint J = jc_joint(tab, nb, nq, nqd, body, s, rows);
  float *q = out + (size_t)set * (nq + nqd) + J.qs, *qd = out + (size_t)set * (nq + nqd) + nq + J.qds;
  if (J.type == PD_JOINT_FREE) {
    const v3 x = qrot_inv(J.q_wj, s.p - J.p_wj), wl = qrot_inv(J.q_wj, J.w_err);
    const v3 vl = qrot_inv(J.q_wj, (s.v - J.v_p) - cross(J.w_err, J.com));
    q[0] = x.x; q[1] = x.y; q[2] = x.z; q[3] = J.r_err.x; q[4] = J.r_err.y; q[5] = J.r_err.z; q[6] = J.r_err.w;
    qd[0] = wl.x; qd[1] = wl.y; qd[2] = wl.z; qd[3] = vl.x; qd[4] = vl.y; qd[5] = vl.z;
  } else if (J.type == PD_JOINT_REVOLUTE) {
    q[0] = twist_angle(dot(qvec(J.r_err), J.axis), J.r_err.w, length(J.axis));
    qd[0] = dot(J.w_err, qrot(J.q_wj, J.axis));
  } else if (J.type == PD_JOINT_COMPOUND) {
    JcCompound C;
    jc_compound(J, generalized, C);
#pragma unroll
    for (int k = 0; k < 3; ++k) { q[k] = C.ang[k]; qd[k] = C.qd[k]; }
  }
}

__global__ __launch_bounds__(256) void k_joint_coords_vjp(int nsets, int nb, const float *__restrict__ tab, const float *__restrict__ state,
                                                          const float *__restrict__ g_out, float *__restrict__ g_b) {
  __shared__ float slot[256 * PD_ADJ];  // lane -> the parent-side adjoint of its joint (odd stride: distinct banks)
  const SetLane L = set_lane(nsets, nb);
  const int set_l = L.set_l, body = L.body;
  const long long set = L.set;
  const bool active = L.active;
  const int nq = (int)tab[1], nqd = (int)tab[2];
  const bool generalized = tab[3] != 0.0f;
  BodyAdj own = adj_zero(), par = adj_zero();
  if (active) {
    const float *rows = state + (size_t)set * nb * PD_ADJ;
    const BodyState s = load_state0(rows, (size_t)body);
    const JcJoint J = jc_joint(tab, nb, nq, nqd, body, s, rows);
    const float *gq = g_out + (size_t)set * (nq + nqd) + J.qs, *gqd = g_out + (size_t)set * (nq + nqd) + nq + J.qds;
    qt adj_r_err = Q4(0, 0, 0, 0), adj_q_wj = adj_r_err;
    v3 adj_w_err = V3(0, 0, 0), adj_p_wj = adj_w_err;
    if (J.type == PD_JOINT_FREE) {
      v3 adj_d = V3(0, 0, 0), adj_l = adj_d;
      adj_qrot_inv(J.q_wj, s.p - J.p_wj, adj_q_wj, adj_d, ld3(gq));
      own.p += adj_d; adj_p_wj -= adj_d;
      adj_r_err += ld4(gq + 3);
      adj_qrot_inv(J.q_wj, J.w_err, adj_q_wj, adj_w_err, ld3(gqd));
      adj_qrot_inv(J.q_wj, (s.v - J.v_p) - cross(J.w_err, J.com), adj_q_wj, adj_l, ld3(gqd + 3));
      own.v += adj_l; par.v -= adj_l;
      adj_cross_a(J.com, adj_w_err, -adj_l);
    } else if (J.type == PD_JOINT_REVOLUTE) {
      float dq_dda, dq_dw;
      (void)twist_angle(dot(qvec(J.r_err), J.axis), J.r_err.w, length(J.axis), dq_dda, dq_dw);
      const float adj_da = gq[0] * dq_dda;
      adj_r_err.x += J.axis.x * adj_da; adj_r_err.y += J.axis.y * adj_da; adj_r_err.z += J.axis.z * adj_da;
      adj_r_err.w += gq[0] * dq_dw;
      adj_w_err += qrot(J.q_wj, J.axis) * gqd[0];
      adj_qrot_q(J.q_wj, J.axis, adj_q_wj, J.w_err * gqd[0]);
    } else if (J.type == PD_JOINT_COMPOUND) {
      JcCompound C;
      jc_compound(J, generalized, C);
      float gm[3] = {gqd[0], gqd[1], gqd[2]}, g_s = 0.0f;
      if (generalized) {  // qd_0 = (m_0 - s m_2) id, qd_2 = (m_2 - s m_0) id, id = 1 / (1 - s^2)
        g_s = (gqd[0] * (2.0f * C.s * C.qd[0] - C.m[2]) + gqd[2] * (2.0f * C.s * C.qd[2] - C.m[0])) * C.id;
        gm[0] = (gqd[0] - C.s * gqd[2]) * C.id;
        gm[2] = (gqd[2] - C.s * gqd[0]) * C.id;
      }
      const v3 adj_u = V3(gm[0], 0, 0) + C.a1 * gm[1] + C.a2 * gm[2];
      v3 adj_a1 = C.u * gm[1], adj_a2 = C.u * gm[2];
      adj_a2.x += g_s;
      qt adj_q_w = Q4(0, 0, 0, 0);
      adj_qrot_inv(C.q_w, J.w_err, adj_q_w, adj_w_err, adj_u);
      adj_qmul_a(J.q_off, adj_q_wj, adj_q_w);
      float adj_ang[3] = {gq[0], gq[1], gq[2]};
      qt adj_q10 = Q4(0, 0, 0, 0), adj_q_1 = adj_q10, adj_q_0 = adj_q10;
      adj_qrot_q(C.q10, V3(0, 0, 1), adj_q10, adj_a2);
      adj_qmul(C.q_1, C.q_0, adj_q_1, adj_q_0, adj_q10);
      adj_q_axis_angle(C.a1, C.ang[1], adj_a1, adj_ang[1], adj_q_1);
      adj_qrot_q(C.q_0, V3(0, 1, 0), adj_q_0, adj_a1);
      adj_q_axis_angle_ang(V3(1, 0, 0), C.ang[0], adj_ang[0], adj_q_0);
      qt adj_q_pc = Q4(0, 0, 0, 0), adj_qa = adj_q_pc;
      quat_decompose_adj(C.q_pc, C.c0, C.c1, C.c2, adj_ang, adj_q_pc);
      adj_qmul_a(J.q_off, adj_qa, adj_q_pc);
      adj_qmul_b(qconj(J.q_off), adj_r_err, adj_qa);
    }
    own.w += adj_w_err; par.w -= adj_w_err;
    qt adj_cq = Q4(0, 0, 0, 0);
    adj_qmul(qconj(J.q_wj), s.r, adj_cq, own.r, adj_r_err);
    adj_q_wj += qconj(adj_cq);
    if (J.parent >= 0) {
      adj_qmul_a(J.q_pj, par.r, adj_q_wj);
      par.p += adj_p_wj;
      adj_qrot_q(J.qp, J.p_pj, par.r, adj_p_wj);
    }
  }
  adj_store(slot + threadIdx.x * PD_ADJ, par);
  __syncthreads();
  if (!active) return;
  const float *B = tab + JC_HEAD + JC_BODY * body, *ch = tab + JC_HEAD + JC_BODY * nb + JC_MAXCH * body;
  const int nch = (int)tab[0] == nb ? min((int)B[21], (int)JC_MAXCH) : 0;
  for (int k = 0; k < nch; ++k) {
    const int c = (int)ch[k];
    if (c >= 0 && c < nb) adj_add_from(own, slot + (set_l * nb + c) * PD_ADJ);
  }
  float o[PD_ADJ];
  adj_store(o, own);
  float *dst = g_b + ((size_t)set * nb + body) * PD_ADJ;
#pragma unroll
  for (int k = 0; k < PD_ADJ; ++k) dst[k] = o[k];
}

// ---- PD_POSE_CENTROIDAL: the whole-body quantities of a state set -- total mass M, centre of mass c and its velocity c_dot, linear
// momentum P, angular momentum L ABOUT c, kinetic energy T and potential energy V -- and their vector-Jacobian product with respect to
// the state rows, the masses and the body-frame inertias.  Per body i (row = p, q xyzw, w, v, m, I row-major; com_i, gravity: the table):
//   x_i = p_i + qrot(q_i, com_i)      wb_i = qrot_inv(q_i, w_i)      (quaternions as they are, like the two ops above)
//   M = sum m_i    c = sum m_i x_i / M    P = sum m_i v_i    c_dot = P / M
//   L = sum [ qrot(q_i, I_i wb_i) + m_i (x_i - c) x (v_i - c_dot) ]
//   T = sum [ m_i |v_i|^2 / 2 + wb_i . I_i wb_i / 2 ]             V = -sum m_i gravity . x_i
// Mapping (k_joint_coords_vjp's): 256 / nb whole state sets per workgroup, a lane per body.  Two stages: (m, m x, m v) per lane into LDS,
// reduced per set; after the barrier every body reads its set's M, c, c_dot and forms its share of (L, T, V) RELATIVE to them (the
// one-pass form sum m x x v - M c x c_dot cancels two terms of size M |c| |c_dot|: 250 ulps at 50 m); second reduction; lane 0 of the set
// stores the 16 floats.  Reduction: a strided tree over the next power of two >= nb on the index of the body INSIDE its set -- depth
// log2, a fixed order that depends on nb alone, so a set's bits do not depend on the run, on n or on where the set sits in the launch.
// No atomics.  LDS slots have odd strides (7 and 5 floats: distinct banks).  The VJP repeats stage one and evaluates the closed-form
// adjoint per body; the orbital term's derivative through c and c_dot vanishes (sum m_i (x_i - c) = sum m_i (v_i - c_dot) = 0), the one
// through m_i does not.  The inertia is taken as ANY 3x3 matrix (raw partials: no symmetry assumed).
// Mass table: include/ppr_diffphys.h (hip_backend.mass_table builds it).  A table of another nb: zeros are written, no row of it is read.
enum { CT_HEAD = 8, CT_BODY = 4, CT_ROW = 23, CT_OUT = 16, CT_MAXNB = 256, CT_S1 = 7, CT_S2 = 5 };
struct CtBody { qt q; v3 w, v, x; float m, I[9]; };
struct CtTotals { float M; v3 c, cd, P; };
__device__ __forceinline__ CtBody ct_load(const float *tab, int body, const float *r) {
  CtBody B;
  B.q = ld4(r + 3); B.w = ld3(r + 7); B.v = ld3(r + 10); B.m = r[13];
#pragma unroll
  for (int k = 0; k < 9; ++k) B.I[k] = r[14 + k];
  B.x = ld3(r) + qrot(B.q, ld3(tab + CT_HEAD + CT_BODY * body));
  return B;
}
// Adds the W-float slots of each set's bodies into the slot of its body 0: lane `body` takes the slot `off` above its own while that one
// is inside the set.  Every lane of the workgroup passes every barrier (the trip count depends on nb alone).
template <int W>
__device__ __forceinline__ void ct_reduce(float *slot, int nb, int body, bool in_set) {
  int p2 = 1;
  while (p2 < nb) p2 <<= 1;
  for (int off = p2 >> 1; off > 0; off >>= 1) {
    __syncthreads();
    if (in_set && body < off && body + off < nb) {
      float *mine = slot + threadIdx.x * W;
      const float *other = slot + (threadIdx.x + off) * W;
#pragma unroll
      for (int k = 0; k < W; ++k) mine[k] += other[k];
    }
  }
  __syncthreads();
}
// Stage one, shared by the two kernels: the lane's (m, m x, m v) into its slot, the per-set reduction, the set's totals.
__device__ __forceinline__ CtTotals ct_stage1(float *s1, int nb, int set_l, int body, bool in_set, bool active, const CtBody &B) {
  float *mine = s1 + threadIdx.x * CT_S1;
  const v3 mx = active ? B.x * B.m : V3(0, 0, 0), mv = active ? B.v * B.m : V3(0, 0, 0);
  mine[0] = active ? B.m : 0.0f;
  mine[1] = mx.x; mine[2] = mx.y; mine[3] = mx.z; mine[4] = mv.x; mine[5] = mv.y; mine[6] = mv.z;
  ct_reduce<CT_S1>(s1, nb, body, in_set);
  CtTotals S;
  S.M = 0.0f; S.c = V3(0, 0, 0); S.cd = S.c; S.P = S.c;
  if (active) {
    const float *t = s1 + set_l * nb * CT_S1;
    S.M = t[0]; S.P = ld3(t + 4);
    S.c = V3(t[1] / S.M, t[2] / S.M, t[3] / S.M);
    S.cd = V3(S.P.x / S.M, S.P.y / S.M, S.P.z / S.M);
  }
  return S;
}

__global__ __launch_bounds__(256) void k_centroidal_fwd(int nsets, int nb, const float *__restrict__ tab, const float *__restrict__ rows,
                                                        float *__restrict__ out) {
  __shared__ float s1[256 * CT_S1], s2[256 * CT_S2];
  const SetLane L = set_lane(nsets, nb);
  const int set_l = L.set_l, body = L.body;
  const long long set = L.set;
  const bool in_set = L.in_set, active = L.active;
  if ((int)tab[0] != nb) {  // not this call's table (the same for every lane of the launch: no barrier is skipped by some)
    if (active && body == 0)
      for (int k = 0; k < CT_OUT; ++k) out[(size_t)set * CT_OUT + k] = 0.0f;
    return;
  }
  CtBody B;
  if (active) B = ct_load(tab, body, rows + ((size_t)set * nb + body) * CT_ROW);
  const CtTotals S = ct_stage1(s1, nb, set_l, body, in_set, active, B);
  float *mine = s2 + threadIdx.x * CT_S2;
#pragma unroll
  for (int k = 0; k < CT_S2; ++k) mine[k] = 0.0f;
  if (active) {
    const v3 g = ld3(tab + 4);
    const v3 wb = qrot_inv(B.q, B.w), h = mat_vec(B.I, wb);
    const v3 l = qrot(B.q, h) + cross(B.x - S.c, B.v - S.cd) * B.m;
    mine[0] = l.x; mine[1] = l.y; mine[2] = l.z;
    mine[3] = 0.5f * B.m * dot(B.v, B.v) + 0.5f * dot(wb, h);
    mine[4] = -B.m * dot(g, B.x);
  }
  ct_reduce<CT_S2>(s2, nb, body, in_set);
  if (active && body == 0) {
    float *o = out + (size_t)set * CT_OUT;
    o[0] = S.M;
    o[1] = S.c.x; o[2] = S.c.y; o[3] = S.c.z;
    o[4] = S.cd.x; o[5] = S.cd.y; o[6] = S.cd.z;
    o[7] = S.P.x; o[8] = S.P.y; o[9] = S.P.z;
#pragma unroll
    for (int k = 0; k < CT_S2; ++k) o[10 + k] = mine[k];
    o[15] = 0.0f;
  }
}

// g_b [n][23]: the raw partials of <g_out, out> with respect to (p, q, w, v, m, I) of every body.
__global__ __launch_bounds__(256) void k_centroidal_vjp(int nsets, int nb, const float *__restrict__ tab, const float *__restrict__ rows,
                                                        const float *__restrict__ g_out, float *__restrict__ g_b) {
  __shared__ float s1[256 * CT_S1];
  const SetLane L = set_lane(nsets, nb);
  const int set_l = L.set_l, body = L.body;
  const long long set = L.set;
  const bool in_set = L.in_set, active = L.active;
  float *dst = g_b + ((size_t)set * nb + body) * CT_ROW;  // (formed, not touched, by an inactive lane)
  if ((int)tab[0] != nb) {
    if (active)
      for (int k = 0; k < CT_ROW; ++k) dst[k] = 0.0f;
    return;
  }
  CtBody B;
  if (active) B = ct_load(tab, body, rows + ((size_t)set * nb + body) * CT_ROW);
  const CtTotals S = ct_stage1(s1, nb, set_l, body, in_set, active, B);
  if (!active) return;
  const float *go = g_out + (size_t)set * CT_OUT;
  const float gM = go[0], gT = go[13], gV = go[14], iM = 1.0f / S.M;
  const v3 gc = ld3(go + 1), gcd = ld3(go + 4), gP = ld3(go + 7), gL = ld3(go + 10);
  const v3 grav = ld3(tab + 4), com = ld3(tab + CT_HEAD + CT_BODY * body);
  const v3 rx = B.x - S.c, rv = B.v - S.cd;
  // x_i: through c, the orbital term and V;  v_i: through c_dot, P, the orbital term and T;  m_i: through all seven
  const v3 adj_x = (gc * iM + cross(rv, gL) - grav * gV) * B.m;
  const v3 adj_v = (gcd * iM + gP + cross(gL, rx) + B.v * gT) * B.m;
  const float adj_m = gM + (dot(gc, rx) + dot(gcd, rv)) * iM + dot(gP, B.v) + dot(gL, cross(rx, rv)) + 0.5f * gT * dot(B.v, B.v) - gV * dot(grav, B.x);
  qt adj_q = Q4(0, 0, 0, 0);
  adj_qrot_q(B.q, com, adj_q, adj_x);  // x = p + qrot(q, com)
  // spin = qrot(q, h), h = I wb, wb = qrot_inv(q, w); T's rotational half wb . I wb / 2
  const v3 wb = qrot_inv(B.q, B.w), h = mat_vec(B.I, wb);
  const v3 adj_h = qrot_inv(B.q, gL);
  adj_qrot_q(B.q, h, adj_q, gL);
  const v3 adj_wb = matT_vec(B.I, adj_h) + (h + matT_vec(B.I, wb)) * (0.5f * gT);
  v3 adj_w = V3(0, 0, 0);
  adj_qrot_inv(B.q, B.w, adj_q, adj_w, adj_wb);
  const v3 ai = adj_h + wb * (0.5f * gT);  // d / d I[j][k] = ai_j wb_k
  dst[0] = adj_x.x; dst[1] = adj_x.y; dst[2] = adj_x.z;
  dst[3] = adj_q.x; dst[4] = adj_q.y; dst[5] = adj_q.z; dst[6] = adj_q.w;
  dst[7] = adj_w.x; dst[8] = adj_w.y; dst[9] = adj_w.z;
  dst[10] = adj_v.x; dst[11] = adj_v.y; dst[12] = adj_v.z;
  dst[13] = adj_m;
  dst[14] = ai.x * wb.x; dst[15] = ai.x * wb.y; dst[16] = ai.x * wb.z;
  dst[17] = ai.y * wb.x; dst[18] = ai.y * wb.y; dst[19] = ai.y * wb.z;
  dst[20] = ai.z * wb.x; dst[21] = ai.z * wb.y; dst[22] = ai.z * wb.z;
}

// ---- PD_POSE_CONTACT_STATE: the ground-contact geometry of every body of a state set -- the height of its lowest candidate, where that
// candidate is and how fast it moves, and how many candidates touch and how deep -- and its vector-Jacobian product with respect to the
// state rows.  Per candidate c of the body (P_c = (x, y, z, dist) and com: the contact table; cv = the cull vector stage_record makes):
//   h_c = contact_height(cv, P_c)      the rollouts' height, bit for bit, and with it their touch decision !(h_c > 0)
//   rp = qrot(q, P_c.xyz), rc = rotm(q) com;  rr_c = (rp.x - rc.x, h_c - p.y - rc.y, rp.z - rc.z);  u_c = v + w x rr_c
// (cp, rr, dpdt of contact_point_fwd).  out [8] = (h, x, z, u.xyz, s, k): c* = the candidate of lowest h_c, lowest table index on ties;
// h = h_c*, (x, z) = (p.x + rp*.x, p.z + rp*.z), u = u_c*; k = the number of touching candidates (as a float), s = the sum of -h_c over them.  A body
// without candidates: (+inf, 0, 0, 0, 0, 0, 0, 0).  A NaN height is never a minimum (strict <), so a non-finite row has a defined
// winner or none -- it reads no candidate outside its body's range.
// Mapping (the ground wrench's): one wavefront per element, four per workgroup; lanes stride over the body's candidates keeping a running
// (h, index) and partial sums, then a six-step xor butterfly -- wave_sum for the sums, wave_argmin for the winner -- after which every
// lane holds the same winner and forms the outputs from it.  No bounding-sphere early-out (the height is wanted for bodies in the
// air), no LDS, no atomics, no barrier: an element's bits depend neither on the run nor on n nor on its place in the launch.
enum { CS_OUT = 8, CS_NONE = 0x7fffffff };
struct CsBody { BodyState s; v3 rc; float4 cv; float Rm[9]; const float4 *pts; int count; };
// Element i's state, cull vector and candidate range.  A table of another nb, or a range that leaves the table's nc candidates, reads
// no candidate (count 0) -- the host cannot validate a device buffer.
__device__ __forceinline__ CsBody cs_stage(const float *tab, int nb, int body, const float *state, size_t i, v3 &com) {
  CsBody C;
  C.s = load_state0(state, i);
  rotm(C.s.r, C.Rm);
  C.cv = make_float4(C.s.p.y, C.Rm[3], C.Rm[4], C.Rm[5]);  // (stage_record)
  com = V3(0, 0, 0); C.rc = com; C.pts = nullptr; C.count = 0;
  if ((int)tab[0] != nb) return C;
  const GwTable T = gw_table(tab);
  const float *B = T.body + GW_BODY * body;
  com = ld3(B);
  C.rc = mat_vec(C.Rm, com);
  const int first = (int)B[3], count = (int)B[4], nc = (int)tab[1];
  if (first >= 0 && count > 0 && first <= nc && count <= nc - first) { C.pts = T.pts + first; C.count = count; }
  return C;
}
// rr of the winner: contact_point_fwd's cp - (p + rc) with p.x and p.z taken out of both sides before the subtraction -- the same
// function, without the cancellation of two numbers of the size of the body's distance from the origin.
__device__ __forceinline__ v3 cs_arm(const CsBody &C, v3 rp, float h) { return V3(rp.x - C.rc.x, (h - C.s.p.y) - C.rc.y, rp.z - C.rc.z); }
// The lower (h, k) pair of the wave in every lane: the lower height, on equal heights the lower index.  h is never NaN (see above), so
// the pairs are totally ordered and both lanes of an exchange keep the same one.
__device__ __forceinline__ void wave_argmin(float &h, int &k) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float oh = __shfl_xor(h, off);
    const int ok = __shfl_xor(k, off);
    const bool take = oh < h || (oh == h && ok < k);
    h = take ? oh : h; k = take ? ok : k;
  }
}
// The sweep both kernels run: the winner and, over the touching candidates, their number, the sum of -h and (SUMS) the sum of P.xyz.
template <bool SUMS>
__device__ __forceinline__ void cs_sweep(const CsBody &C, int lane, float &h, int &k, float &depth, float &touching, v3 &sumP) {
  h = INFINITY; k = CS_NONE; depth = 0.f; touching = 0.f; sumP = V3(0, 0, 0);
  for (int c = lane; c < C.count; c += 64) {
    const float4 P = C.pts[c];
    const float hc = contact_height(C.cv, P);
    if (hc < h) { h = hc; k = c; }
    if (!(hc > 0.0f)) {
      depth -= hc; touching += 1.0f;
      if (SUMS) sumP += V3(P.x, P.y, P.z);
    }
  }
  wave_argmin(h, k);
  depth = wave_sum(depth); touching = wave_sum(touching);
  if (SUMS) { sumP.x = wave_sum(sumP.x); sumP.y = wave_sum(sumP.y); sumP.z = wave_sum(sumP.z); }
}

__global__ __launch_bounds__(256) void k_contact_state_fwd(int n, int nb, const float *__restrict__ tab, const float *__restrict__ state,
                                                           float *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  v3 com, sumP;
  const CsBody C = cs_stage(tab, nb, (int)(i % nb), state, (size_t)i, com);
  float h, depth, touching;
  int k;
  cs_sweep<false>(C, lane, h, k, depth, touching, sumP);
  float o[CS_OUT] = {INFINITY, 0.f, 0.f, 0.f, 0.f, 0.f, depth, touching};
  if (k != CS_NONE) {  // (k < C.count: an index some lane swept)
    const float4 P = C.pts[k];
    const v3 rp = qrot(C.s.r, V3(P.x, P.y, P.z));
    const v3 u = C.s.v + cross(C.s.w, cs_arm(C, rp, h));
    o[0] = h; o[1] = C.s.p.x + rp.x; o[2] = C.s.p.z + rp.z; o[3] = u.x; o[4] = u.y; o[5] = u.z;
  }
  if (lane < CS_OUT) {
    float v = o[0];
#pragma unroll
    for (int j = 1; j < CS_OUT; ++j) v = lane == j ? o[j] : v;
    out[(size_t)i * CS_OUT + lane] = v;
  }
}

// g_b [n][13]: the raw partials of <g_out, out> with respect to the state row (quaternion entries not projected; g_out[7], the count's,
// is ignored).  Through c*, found again with the forward kernel's bits, and through s: d s / d p.y = -k and d s / d q = the row-1 adjoint
// of rotm applied to -sum_touching P_c.xyz.  Every rotation by q is rotm(q) (pd_math.h), so the quaternion adjoint is ONE matrix adjoint:
// rows 0 and 2 from rp and rc, row 1 from the heights and rc, then one rotm_adj.
__global__ __launch_bounds__(256) void k_contact_state_vjp(int n, int nb, const float *__restrict__ tab, const float *__restrict__ state,
                                                           const float *__restrict__ g_out, float *__restrict__ g_b) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  v3 com, sumP;
  const CsBody C = cs_stage(tab, nb, (int)(i % nb), state, (size_t)i, com);
  float h, depth, touching;
  int k;
  cs_sweep<true>(C, lane, h, k, depth, touching, sumP);
  float acc[PD_ADJ];
#pragma unroll
  for (int j = 0; j < PD_ADJ; ++j) acc[j] = 0.f;
  if (k != CS_NONE) {
    const float *g = g_out + (size_t)i * CS_OUT;
    const float g_h = g[0], g_x = g[1], g_z = g[2], g_s = g[6];
    const v3 g_u = ld3(g + 3);
    const float4 P = C.pts[k];
    const v3 cpt = V3(P.x, P.y, P.z);
    const v3 rp = qrot(C.s.r, cpt);
    const v3 rr = cs_arm(C, rp, h);
    BodyAdj o = adj_zero();
    v3 adj_rr = V3(0, 0, 0);
    o.v = g_u;
    adj_cross(C.s.w, rr, o.w, adj_rr, g_u);                      // u = v + w x rr
    // rr does not depend on p (p.y enters h and leaves rr.y again): p sees x, z, h and s = -sum_touching h_c alone
    o.p = V3(g_x, g_h - g_s * touching, g_z);
    float aM[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) aM[j] = 0.f;
    add_outer(aM, V3(adj_rr.x + g_x, adj_rr.y + g_h, adj_rr.z + g_z), cpt);  // rp = rotm(q) P.xyz (rows 0, 2), h = p.y + row1 . P - dist (row 1)
    add_outer(aM, -adj_rr, com);                                 // rc = rotm(q) com
    add_outer(aM, V3(0.f, -g_s, 0.f), sumP);
    rotm_adj(C.s.r, aM, o.r);
    adj_store(acc, o);
  }
  if (lane < PD_ADJ) {
    float v = acc[0];
#pragma unroll
    for (int j = 1; j < PD_ADJ; ++j) v = lane == j ? acc[j] : v;
    g_b[(size_t)i * PD_ADJ + lane] = v;
  }
}

// ---- PD_POSE_JOINT_WRENCH: the joint pass's contribution to body_f (eval_body_joints, integrator_euler.py:289-451; joint_fwd,
// pd_device.h) as a function of ONE state set and the joints' controls, and its vector-Jacobian product with respect to the state rows
// and the controls.  Joint i = child body i pulls its two bodies with the pair (t_i, f_i):
//   out_i = -(t_i + r_c,i x f_i, f_i) + sum over the children c of i (t_c + r_p,c x f_c, f_c)     own joint first, then the table's child order
//   FIXED     t = R(q_wj) (v h) ake + w_err akd ads,  v h = fixed_ang_h: the scale-invariant 2 acos(w) normalize(v) of r_err = (v, w)
//   REVOLUTE  t = axis_p jf + (axis_p x axis_c) ake + (w_err - axis_p qd) akd ads,  jf = joint_force(twist_angle, qd = w_err . axis_p, slot 0)
//   COMPOUND  t = clamp3(sum_k axw_k joint_force(ang_k, axw_k . w_err, slot k), 1e4) on jc_compound's angles, axes and measured rates
//   f = x_err ake + v_err akd (COMPOUND: clamp3(., 1e4));  ads = 0.01;  FREE: no pair
// The lever arms and the position error are formed without the rollout's cancellation of two numbers of the size of the body's distance
// from the origin -- r_c = -R(q_c) com_c, r_p = R(q_p) (p_pj - com_p), x_err = (p_c - p_p) - R(q_p) p_pj: the same functions (the contact
// state's cs_arm takes the same liberty).  Default numeric policy only, like the joint coordinates.
// Rows [n][25]: the state (13), then the joint's controls in dof slots k = 0..2: act 13 + k, target 16 + k, ke 19 + k, kd 22 + k; a
// REVOLUTE joint uses slot 0, a COMPOUND joint all three, FIXED / FREE none; an unused slot never enters arithmetic (a select keeps it
// out) and its gradient is written as 0.  Table: the joint table (rate mode measured) followed by (attach_ke, attach_kd, 0, 0) and 12
// floats per body, (lo, up, limit_ke, limit_kd) per slot.
// Mapping: a lane per body, whole state sets per workgroup (set_lane).  Forward: a lane leaves the parent-side wrench of its joint in an
// LDS slot of 6 floats (stride 7) and, after ONE barrier, adds its children's slots in the table's child order to its own side.  VJP: a
// lane reads g_out of its own row and of its parent's, runs its joint's adjoint and hands the parent-side state adjoint over as
// k_joint_coords_vjp does.  No atomics: a set's bits depend neither on the run nor on n nor on its place in the launch.
enum { JW_ROW = 25, JW_HEAD = 4, JW_BODY = 12, JW_S = 7 };
struct JwJoint {  // a joint's pair and what its adjoint needs of the forward pass
  JcJoint J;
  JcCompound C;
  bool pulls;                                   // FIXED, REVOLUTE or COMPOUND: the joint has a pair
  float act[3], tgt[3], ke[3], kd[3], jf[3];    // the used slots' controls (0 in an unused slot) and joint forces
  const float *lim;                             // the body's 3 x (lo, up, limit_ke, limit_kd)
  float ake, akd;
  v3 r_c, r_p, x_err, v_err, f_raw, t_raw, t, f;
  v3 axis_p, axis_c, axw[3];
  float q, qd, dq_dda, dq_dw;                   // REVOLUTE
};
// tab[0] == nb is the caller's to check: a table of another nb has no row for this body.
__device__ __forceinline__ void jw_eval(const float *tab, int nb, int body, const BodyState &s, const float *set_rows, JwJoint &W) {
  W.J = jc_joint<JW_ROW>(tab, nb, (int)tab[1], (int)tab[2], body, s, set_rows);
  const JcJoint &J = W.J;
  const float *ext = tab + JC_HEAD + (JC_BODY + JC_MAXCH) * nb;
  W.ake = ext[0]; W.akd = ext[1];
  W.lim = ext + JW_HEAD + JW_BODY * body;
  const float ake = W.ake, akd = W.akd, ads = 0.01f;
  const int nd = J.type == PD_JOINT_REVOLUTE ? 1 : J.type == PD_JOINT_COMPOUND ? 3 : 0;
  const float *c = set_rows + (size_t)body * JW_ROW + PD_ADJ;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const bool used = k < nd;
    W.act[k] = used ? c[k] : 0.0f; W.tgt[k] = used ? c[3 + k] : 0.0f; W.ke[k] = used ? c[6 + k] : 0.0f; W.kd[k] = used ? c[9 + k] : 0.0f;
    W.jf[k] = 0.0f;
  }
  const v3 zero = V3(0, 0, 0);
  W.r_c = zero; W.r_p = zero; W.x_err = zero; W.v_err = zero; W.f_raw = zero; W.t_raw = zero; W.t = zero; W.f = zero;
  W.pulls = J.type == PD_JOINT_FIXED || J.type == PD_JOINT_REVOLUTE || J.type == PD_JOINT_COMPOUND;
  if (!W.pulls) return;  // FREE (:382)
  W.r_c = -qrot(s.r, J.com);
  W.x_err = s.p - J.p_pj;
  if (J.parent >= 0) {
    const v3 com_p = ld3(tab + JC_HEAD + JC_BODY * J.parent + 18);
    W.r_p = qrot(J.qp, J.p_pj - com_p);
    W.x_err = (s.p - J.pp) - qrot(J.qp, J.p_pj);
  }
  W.v_err = s.v - J.v_p;
  W.f_raw = W.x_err * ake + W.v_err * akd;
  W.f = W.f_raw;
  if (J.type == PD_JOINT_FIXED) {  // :385-390
    float hss_, hw_;
    const v3 rv = qvec(J.r_err);
    const v3 ang_err = rv * fixed_ang_h(dot(rv, rv), J.r_err.w, hss_, hw_);
    W.t_raw = qrot(J.q_wj, ang_err) * ake + J.w_err * (akd * ads);
    W.t = W.t_raw;
  } else if (J.type == PD_JOINT_REVOLUTE) {  // :392-409
    W.axis_p = qrot(J.q_wj, J.axis); W.axis_c = qrot(s.r, J.axis);
    W.q = twist_angle(dot(qvec(J.r_err), J.axis), J.r_err.w, length(J.axis), W.dq_dda, W.dq_dw);
    W.qd = dot(J.w_err, W.axis_p);
    W.jf[0] = joint_force(W.q, W.qd, W.tgt[0], W.ke[0], W.kd[0], W.act[0], W.lim[0], W.lim[1], W.lim[2], W.lim[3]);
    W.t_raw = W.axis_p * W.jf[0];
    W.t_raw += cross(W.axis_p, W.axis_c) * ake + (J.w_err - W.axis_p * W.qd) * (akd * ads);
    W.t = W.t_raw;
  } else {  // COMPOUND :411-445
    jc_compound(J, false, W.C);
    const v3 ax[3] = {V3(1, 0, 0), W.C.a1, W.C.a2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float *L = W.lim + 4 * k;
      W.axw[k] = qrot(W.C.q_w, ax[k]);
      W.jf[k] = joint_force(W.C.ang[k], W.C.m[k], W.tgt[k], W.ke[k], W.kd[k], W.act[k], L[0], L[1], L[2], L[3]);
      W.t_raw += W.axw[k] * W.jf[k];
    }
    W.t = clamp3(W.t_raw, 1.0e4f);
    W.f = clamp3(W.f_raw, 1.0e4f);
  }
}

__global__ __launch_bounds__(256) void k_joint_wrench_fwd(int nsets, int nb, const float *__restrict__ tab, const float *__restrict__ rows,
                                                          float *__restrict__ out) {
  __shared__ float slot[256 * JW_S];  // lane -> the parent-side wrench of its joint (odd stride: distinct banks)
  const SetLane L = set_lane(nsets, nb);
  const bool mine = (int)tab[0] == nb;  // not this call's table: no row of it is read, zeros
  v3 own_t = V3(0, 0, 0), own_f = own_t, par_t = own_t, par_f = own_t;
  if (L.active && mine) {
    const float *set_rows = rows + (size_t)L.set * nb * JW_ROW;
    const BodyState s = load_row<JW_ROW>(set_rows, (size_t)L.body);
    JwJoint W;
    jw_eval(tab, nb, L.body, s, set_rows, W);
    own_t = -(W.t + cross(W.r_c, W.f)); own_f = -W.f;  // :451
    if (W.J.parent >= 0) { par_t = W.t + cross(W.r_p, W.f); par_f = W.f; }  // :448-449
  }
  float *mine_s = slot + threadIdx.x * JW_S;
  mine_s[0] = par_t.x; mine_s[1] = par_t.y; mine_s[2] = par_t.z; mine_s[3] = par_f.x; mine_s[4] = par_f.y; mine_s[5] = par_f.z;
  __syncthreads();
  if (!L.active) return;
  if (mine) {
    const float *B = tab + JC_HEAD + JC_BODY * L.body, *ch = tab + JC_HEAD + JC_BODY * nb + JC_MAXCH * L.body;
    const int nch = min((int)B[21], (int)JC_MAXCH);
    for (int k = 0; k < nch; ++k) {
      const int c = (int)ch[k];
      if (c >= 0 && c < nb) {
        const float *cs = slot + (L.set_l * nb + c) * JW_S;
        own_t += ld3(cs); own_f += ld3(cs + 3);
      }
    }
  }
  float *dst = out + ((size_t)L.set * nb + L.body) * 6;
  dst[0] = own_t.x; dst[1] = own_t.y; dst[2] = own_t.z; dst[3] = own_f.x; dst[4] = own_f.y; dst[5] = own_f.z;
}

// g_b [n][25]: the raw partials of <g_out, out> with respect to the state row (quaternion entries not projected) and the twelve control
// slots.  Joint i sees -g_out[i] on its child side and +g_out[parent] on its parent side (the adjoint of joint_adj_apply, pd_device.h,
// on the lever arms and the position error as jw_eval forms them); limits, attachment gains and the table have no gradient.
__global__ __launch_bounds__(256) void k_joint_wrench_vjp(int nsets, int nb, const float *__restrict__ tab, const float *__restrict__ rows,
                                                          const float *__restrict__ g_out, float *__restrict__ g_b) {
  __shared__ float slot[256 * PD_ADJ];  // lane -> the parent-side state adjoint of its joint (odd stride: distinct banks)
  const SetLane L = set_lane(nsets, nb);
  const bool mine = (int)tab[0] == nb;
  BodyAdj own = adj_zero(), par = adj_zero();
  float a_act[3] = {0.f, 0.f, 0.f}, a_tgt[3] = {0.f, 0.f, 0.f}, a_ke[3] = {0.f, 0.f, 0.f}, a_kd[3] = {0.f, 0.f, 0.f};
  if (L.active && mine) {
    const float *set_rows = rows + (size_t)L.set * nb * JW_ROW;
    const BodyState s = load_row<JW_ROW>(set_rows, (size_t)L.body);
    JwJoint W;
    jw_eval(tab, nb, L.body, s, set_rows, W);
    const JcJoint &J = W.J;
    if (W.pulls) {
      const float ake = W.ake, akd = W.akd, ads = 0.01f;
      const float *g = g_out + ((size_t)L.set * nb + L.body) * 6;
      const v3 gc_t = ld3(g), gc_f = ld3(g + 3);
      v3 adj_t = -gc_t, adj_f = -gc_f, adj_r_c = V3(0, 0, 0), adj_r_p = adj_r_c;
      adj_cross(W.r_c, W.f, adj_r_c, adj_f, -gc_t);
      if (J.parent >= 0) {
        const float *gp = g_out + ((size_t)L.set * nb + J.parent) * 6;
        const v3 gp_t = ld3(gp), gp_f = ld3(gp + 3);
        adj_t += gp_t; adj_f += gp_f;
        adj_cross(W.r_p, W.f, adj_r_p, adj_f, gp_t);
      }
      v3 adj_x_err = V3(0, 0, 0), adj_v_err = adj_x_err, adj_w_err = adj_x_err;
      qt adj_r_err = Q4(0, 0, 0, 0), adj_q_wj = adj_r_err;
      if (J.type == PD_JOINT_FIXED) {
        const v3 rv = qvec(J.r_err);
        float hss, h_w;
        const float h = fixed_ang_h(dot(rv, rv), J.r_err.w, hss, h_w);
        adj_x_err += adj_f * ake; adj_v_err += adj_f * akd; adj_w_err += adj_t * (akd * ads);
        v3 adj_ang_err = V3(0, 0, 0);
        adj_qrot(J.q_wj, rv * h, adj_q_wj, adj_ang_err, adj_t * ake);
        const float va = dot(rv, adj_ang_err);
        const v3 adj_rv = adj_ang_err * h + rv * (va * hss);
        adj_r_err.x += adj_rv.x; adj_r_err.y += adj_rv.y; adj_r_err.z += adj_rv.z;
        adj_r_err.w += va * h_w;
      } else if (J.type == PD_JOINT_REVOLUTE) {
        adj_x_err += adj_f * ake; adj_v_err += adj_f * akd;
        const float adj_jf = dot(adj_t, W.axis_p);
        v3 adj_axis_p = adj_t * W.jf[0], adj_axis_c = V3(0, 0, 0);
        adj_w_err += adj_t * (akd * ads);
        float adj_qd = -dot(adj_t, W.axis_p) * (akd * ads), adj_q = 0.f;
        adj_axis_p += adj_t * (-W.qd * (akd * ads));
        adj_cross(W.axis_p, W.axis_c, adj_axis_p, adj_axis_c, adj_t * ake);
        joint_force_adj(W.q, W.qd, W.tgt[0], W.ke[0], W.kd[0], W.lim[0], W.lim[1], W.lim[2], W.lim[3], adj_jf, adj_q, adj_qd, a_tgt[0],
                        a_ke[0], a_kd[0], a_act[0]);
        adj_w_err += W.axis_p * adj_qd; adj_axis_p += J.w_err * adj_qd;
        const float adj_da = adj_q * W.dq_dda;
        adj_r_err.x += J.axis.x * adj_da; adj_r_err.y += J.axis.y * adj_da; adj_r_err.z += J.axis.z * adj_da;
        adj_r_err.w += adj_q * W.dq_dw;
        adj_qrot_q(J.q_wj, J.axis, adj_q_wj, adj_axis_p);
        adj_qrot_q(s.r, J.axis, own.r, adj_axis_c);
      } else {  // COMPOUND
        const JcCompound &C = W.C;
        const v3 adj_f_raw = clamp3_pass(W.f_raw, adj_f, 1.0e4f);
        adj_x_err += adj_f_raw * ake; adj_v_err += adj_f_raw * akd;
        const v3 adj_t_raw = clamp3_pass(W.t_raw, adj_t, 1.0e4f);
        const v3 ax[3] = {V3(1, 0, 0), C.a1, C.a2};
        float adj_ang[3] = {0.f, 0.f, 0.f}, adj_m[3] = {0.f, 0.f, 0.f};
        v3 adj_ax[3] = {V3(0, 0, 0), V3(0, 0, 0), V3(0, 0, 0)};
        qt adj_q_w = Q4(0, 0, 0, 0);
#pragma unroll
        for (int k = 2; k >= 0; --k) {
          const float *Lm = W.lim + 4 * k;
          joint_force_adj(C.ang[k], C.m[k], W.tgt[k], W.ke[k], W.kd[k], Lm[0], Lm[1], Lm[2], Lm[3], dot(adj_t_raw, W.axw[k]), adj_ang[k],
                          adj_m[k], a_tgt[k], a_ke[k], a_kd[k], a_act[k]);
          adj_qrot(C.q_w, ax[k], adj_q_w, adj_ax[k], adj_t_raw * W.jf[k]);
        }
        // m_k = a_k . u, u = R(q_w)^T w_err; then the axis chain and the decomposition, as k_joint_coords_vjp in rate mode measured
        const v3 adj_u = V3(adj_m[0], 0, 0) + C.a1 * adj_m[1] + C.a2 * adj_m[2];
        v3 adj_a1 = adj_ax[1] + C.u * adj_m[1];
        const v3 adj_a2 = adj_ax[2] + C.u * adj_m[2];
        adj_qrot_inv(C.q_w, J.w_err, adj_q_w, adj_w_err, adj_u);
        adj_qmul_a(J.q_off, adj_q_wj, adj_q_w);
        qt adj_q10 = Q4(0, 0, 0, 0), adj_q_1 = adj_q10, adj_q_0 = adj_q10;
        adj_qrot_q(C.q10, V3(0, 0, 1), adj_q10, adj_a2);
        adj_qmul(C.q_1, C.q_0, adj_q_1, adj_q_0, adj_q10);
        adj_q_axis_angle(C.a1, C.ang[1], adj_a1, adj_ang[1], adj_q_1);
        adj_qrot_q(C.q_0, V3(0, 1, 0), adj_q_0, adj_a1);
        adj_q_axis_angle_ang(V3(1, 0, 0), C.ang[0], adj_ang[0], adj_q_0);
        qt adj_q_pc = Q4(0, 0, 0, 0), adj_qa = adj_q_pc;
        quat_decompose_adj(C.q_pc, C.c0, C.c1, C.c2, adj_ang, adj_q_pc);
        adj_qmul_a(J.q_off, adj_qa, adj_q_pc);
        adj_qmul_b(qconj(J.q_off), adj_r_err, adj_qa);
      }
      qt adj_cq = Q4(0, 0, 0, 0);
      adj_qmul(qconj(J.q_wj), s.r, adj_cq, own.r, adj_r_err);  // r_err = conj(q_wj) q_c
      adj_q_wj += qconj(adj_cq);
      adj_qrot_q(s.r, J.com, own.r, -adj_r_c);                 // r_c = -R(q_c) com
      own.p += adj_x_err; own.w += adj_w_err; own.v += adj_v_err;
      if (J.parent >= 0) {
        const v3 com_p = ld3(tab + JC_HEAD + JC_BODY * J.parent + 18);
        par.p = -adj_x_err; par.w = -adj_w_err; par.v = -adj_v_err;
        adj_qrot_q(J.qp, J.p_pj, par.r, -adj_x_err);           // x_err = (p_c - p_p) - R(q_p) p_pj
        adj_qrot_q(J.qp, J.p_pj - com_p, par.r, adj_r_p);      // r_p = R(q_p) (p_pj - com_p)
        adj_qmul_a(J.q_pj, par.r, adj_q_wj);                   // q_wj = q_p q_pj
      }
    }
  }
  adj_store(slot + threadIdx.x * PD_ADJ, par);
  __syncthreads();
  if (!L.active) return;
  if (mine) {
    const float *B = tab + JC_HEAD + JC_BODY * L.body, *ch = tab + JC_HEAD + JC_BODY * nb + JC_MAXCH * L.body;
    const int nch = min((int)B[21], (int)JC_MAXCH);
    for (int k = 0; k < nch; ++k) {
      const int c = (int)ch[k];
      if (c >= 0 && c < nb) adj_add_from(own, slot + (L.set_l * nb + c) * PD_ADJ);
    }
  }
  float o[JW_ROW];
  adj_store(o, own);
#pragma unroll
  for (int k = 0; k < 3; ++k) { o[13 + k] = a_act[k]; o[16 + k] = a_tgt[k]; o[19 + k] = a_ke[k]; o[22 + k] = a_kd[k]; }
  float *dst = g_b + ((size_t)L.set * nb + L.body) * JW_ROW;
#pragma unroll
  for (int k = 0; k < JW_ROW; ++k) dst[k] = o[k];
}

// ---- PD_POSE_GENERALIZED_FORCE: the generalised joint forces of per-body wrenches -- J^T of the articulation applied to rows
// (p, q xyzw, t, f): per REVOLUTE / COMPOUND dof the projection on its world axis of the subtree's moment about the joint anchor, per
// FREE joint the subtree's net wrench about the child's centre of mass in the joint frame -- and its vector-Jacobian product with
// respect to poses and wrenches.  With x_b = p_b + R(q_b) com_b, F_i = sum_{b in subtree(i)} f_b, N_i(o) = sum (t_b + (x_b - o) x f_b):
//   REVOLUTE  tau = (R_wj axis) . N_i(p_wj)
//   COMPOUND  g_k = (R_wj R_off a_k) . N_i(p_wj) on jc_compound's angles and axes; mode 1 (generalized): tau = g; mode 0 (actuator):
//             tau = G^-1 g, the Gram solve of the rates (tau_1 = g_1, (tau_0, tau_2) = ((g_0 - s g_2), (g_2 - s g_0)) / (1 - s^2))
//   FREE      (R_wj^-1 N_i(x_i), R_wj^-1 F_i);   FIXED: nothing
// Frames, axes, the range checks and the mode float are PD_POSE_JOINT_COORDS' (jc_joint on the joint table, unchanged; the rows' last six
// floats are a wrench, so jc_joint's rates are not looked at).
// Mapping: a lane per body, whole state sets per workgroup (set_lane).  The table holds parents and children, not depths: every lane
// finds its depth by pointer jumping over the parent indices in LDS (log2 nb rounds), the workgroup's largest depth is the trip count of
// the level sweeps -- table data alone, so every barrier sits in workgroup-uniform control flow.  Forward: (F, M) per body in an LDS
// slot, M about o0 = the origin of the set's body 0 (the set's distance from the world origin never enters a product); levels deepest
// first, a body adds its children's slots in the table's child order; then N_i(o) = M_i - (o - o0) x F_i with o - o0 formed from
// differences.  VJP: the sweep again (the axes' adjoints need N_i), the joint's adjoint, an ancestor sum of (adj F, adj M) from the roots
// down, the body's own adjoint, and the parent-side pose adjoint handed over as k_joint_coords_vjp does.  o0 is a constant of the
// adjoint: the function does not depend on it.  No atomics: a set's bits depend neither on the run nor on n nor on its place in the
// launch.  A table of another nb: zeros (out by that table's own nqd), no row of it is read.
enum { GF_S = 7 };  // floats of an LDS slot (6 or 7 used; odd stride: distinct banks)
struct GfTree { int dep, maxd, nch, parent; const float *ch; };
// The lane's parent (inside the set, or -1), children and depth, and the workgroup's largest depth.  Every lane of the workgroup calls
// it: the barriers' count depends on nb alone.  A malformed table (a parent cycle) gives depths that mean nothing but stay below nb.
__device__ __forceinline__ GfTree gf_tree(const float *tab, int nb, const SetLane &L, int (*s_anc)[256], int (*s_dep)[256], int *s_max) {
  GfTree T;
  T.nch = 0; T.ch = tab; T.parent = -1;
  if (L.in_set) {
    const float *B = tab + JC_HEAD + JC_BODY * L.body;
    const int par = (int)B[0];
    T.parent = par >= 0 && par < nb ? par : -1;
    T.nch = min((int)B[21], (int)JC_MAXCH);
    T.ch = tab + JC_HEAD + JC_BODY * nb + JC_MAXCH * L.body;
  }
  int anc = T.parent, dep = anc >= 0 ? 1 : 0, cur = 0;
  for (int span = 1; span < nb; span <<= 1) {  // dep = the distance to anc; anc jumps 2^round bodies up
    s_anc[cur][threadIdx.x] = anc; s_dep[cur][threadIdx.x] = dep;
    __syncthreads();
    if (anc >= 0) {
      const int a = L.set_l * nb + anc;
      dep += s_dep[cur][a]; anc = s_anc[cur][a];
    }
    cur ^= 1;  // the other pair next round: nobody reads it any more
  }
  T.dep = min(dep, nb - 1);
  int m = T.dep;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off));
  if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
  __syncthreads();
  T.maxd = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
  return T;
}
__device__ __forceinline__ void gf_put(float *s, v3 a, v3 b) { s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = b.x; s[4] = b.y; s[5] = b.z; }
// Subtree sums of (F, M): levels deepest first, a body adds its children's slots in the table's child order and publishes its own.
__device__ __forceinline__ void gf_up(float *slot, const GfTree &T, const SetLane &L, int nb, v3 &F, v3 &M) {
  float *mine = slot + threadIdx.x * GF_S;
  gf_put(mine, F, M);
  for (int lev = T.maxd - 1; lev >= 0; --lev) {
    __syncthreads();
    if (L.in_set && T.dep == lev && T.nch > 0) {
      for (int k = 0; k < T.nch; ++k) {
        const int c = (int)T.ch[k];
        if (c >= 0 && c < nb) {
          const float *cs = slot + (L.set_l * nb + c) * GF_S;
          F += ld3(cs); M += ld3(cs + 3);
        }
      }
      gf_put(mine, F, M);
    }
  }
}
struct GfBody { BodyState s; JcJoint J; v3 d, r; };  // d = x_b - o0; r = the joint's anchor - o0 (p_wj, or x_b for a FREE joint)
__device__ __forceinline__ void gf_load(const float *tab, int nb, int body, const float *set_rows, GfBody &B) {
  const v3 o0 = ld3(set_rows);
  B.s = load_state0(set_rows, (size_t)body);  // (s.w, s.v) = (t, f)
  B.J = jc_joint(tab, nb, (int)tab[1], (int)tab[2], body, B.s, set_rows);
  B.J.w_err = V3(0, 0, 0);
  B.d = (B.s.p - o0) + qrot(B.s.r, B.J.com);
  B.r = B.J.type == PD_JOINT_FREE ? B.d : B.J.parent >= 0 ? (B.J.pp - o0) + qrot(B.J.qp, B.J.p_pj) : B.J.p_pj - o0;
}

__global__ __launch_bounds__(256) void k_generalized_force_fwd(int nsets, int nb, const float *__restrict__ tab, const float *__restrict__ rows,
                                                               float *__restrict__ out) {
  __shared__ float slot[256 * GF_S];
  __shared__ int s_anc[2][256], s_dep[2][256], s_max[4];
  const SetLane L = set_lane(nsets, nb);
  const int nqd = (int)tab[2];
  if ((int)tab[0] != nb) {  // not this call's table (the same for every lane of the launch: no barrier is skipped by some)
    if (L.active)
      for (int k = L.body; k < nqd; k += nb) out[(size_t)L.set * nqd + k] = 0.0f;
    return;
  }
  const bool generalized = tab[3] != 0.0f;
  const GfTree T = gf_tree(tab, nb, L, s_anc, s_dep, s_max);
  GfBody B;
  v3 F = V3(0, 0, 0), M = F;
  if (L.active) {
    gf_load(tab, nb, L.body, rows + (size_t)L.set * nb * PD_ADJ, B);
    F = B.s.v; M = B.s.w + cross(B.d, F);
  }
  gf_up(slot, T, L, nb, F, M);
  if (!L.active) return;
  const JcJoint &J = B.J;
  const v3 N = M - cross(B.r, F);
  float *o = out + (size_t)L.set * nqd + J.qds;
  if (J.type == PD_JOINT_FREE) {
    const v3 a = qrot_inv(J.q_wj, N), l = qrot_inv(J.q_wj, F);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = l.x; o[4] = l.y; o[5] = l.z;
  } else if (J.type == PD_JOINT_REVOLUTE) {
    o[0] = dot(qrot(J.q_wj, J.axis), N);
  } else if (J.type == PD_JOINT_COMPOUND) {
    JcCompound C;
    jc_compound(J, false, C);
    const v3 u = qrot_inv(C.q_w, N);  // (R a) . N = a . (R^T N)
    const float g0 = u.x, g1 = dot(C.a1, u), g2 = dot(C.a2, u);
    if (generalized) { o[0] = g0; o[1] = g1; o[2] = g2; }
    else {
      const float id = 1.0f / (1.0f - C.s * C.s);
      o[0] = (g0 - C.s * g2) * id; o[1] = g1; o[2] = (g2 - C.s * g0) * id;
    }
  }
}

// g_b [n][13]: the raw partials of <g_out, out> with respect to (p, q, t, f) of every body.
__global__ __launch_bounds__(256) void k_generalized_force_vjp(int nsets, int nb, const float *__restrict__ tab, const float *__restrict__ rows,
                                                               const float *__restrict__ g_out, float *__restrict__ g_b) {
  __shared__ float slot[256 * GF_S], down[256 * GF_S], pslot[256 * GF_S];  // subtree sums / ancestor sums / the parent-side pose adjoint
  __shared__ int s_anc[2][256], s_dep[2][256], s_max[4];
  const SetLane L = set_lane(nsets, nb);
  float *dst = g_b + ((size_t)L.set * nb + L.body) * PD_ADJ;  // (formed, not touched, by an inactive lane)
  if ((int)tab[0] != nb) {
    if (L.active)
      for (int k = 0; k < PD_ADJ; ++k) dst[k] = 0.0f;
    return;
  }
  const int nqd = (int)tab[2];
  const bool generalized = tab[3] != 0.0f;
  const GfTree T = gf_tree(tab, nb, L, s_anc, s_dep, s_max);
  GfBody B;
  v3 F = V3(0, 0, 0), M = F;
  if (L.active) {
    gf_load(tab, nb, L.body, rows + (size_t)L.set * nb * PD_ADJ, B);
    F = B.s.v; M = B.s.w + cross(B.d, F);
  }
  gf_up(slot, T, L, nb, F, M);
  // the joint's adjoint: (adj F_i, adj M_i) of its subtree sums, the pose adjoints of its own body and of its parent
  v3 aF = V3(0, 0, 0), aM = aF, own_p = aF, par_p = aF, adj_r = aF;
  qt own_q = Q4(0, 0, 0, 0), par_q = own_q;
  if (L.active) {
    const JcJoint &J = B.J;
    const v3 N = M - cross(B.r, F);
    const float *g = g_out + (size_t)L.set * nqd + J.qds;
    qt adj_q_wj = Q4(0, 0, 0, 0);
    v3 adj_N = V3(0, 0, 0);
    if (J.type == PD_JOINT_FREE) {
      adj_qrot_inv(J.q_wj, N, adj_q_wj, adj_N, ld3(g));
      adj_qrot_inv(J.q_wj, F, adj_q_wj, aF, ld3(g + 3));
    } else if (J.type == PD_JOINT_REVOLUTE) {
      adj_N = qrot(J.q_wj, J.axis) * g[0];
      adj_qrot_q(J.q_wj, J.axis, adj_q_wj, N * g[0]);
    } else if (J.type == PD_JOINT_COMPOUND) {
      JcCompound C;
      jc_compound(J, false, C);
      const v3 u = qrot_inv(C.q_w, N);
      const float g0 = u.x, g2 = dot(C.a2, u);
      float gm[3] = {g[0], g[1], g[2]}, g_s = 0.0f;
      if (!generalized) {  // tau_0 = (g_0 - s g_2) id, tau_2 = (g_2 - s g_0) id, id = 1 / (1 - s^2)
        const float id = 1.0f / (1.0f - C.s * C.s);
        const float t0 = (g0 - C.s * g2) * id, t2 = (g2 - C.s * g0) * id;
        g_s = (g[0] * (2.0f * C.s * t0 - g2) + g[2] * (2.0f * C.s * t2 - g0)) * id;
        gm[0] = (g[0] - C.s * g[2]) * id;
        gm[2] = (g[2] - C.s * g[0]) * id;
      }
      const v3 adj_u = V3(gm[0], 0, 0) + C.a1 * gm[1] + C.a2 * gm[2];
      v3 adj_a1 = u * gm[1], adj_a2 = u * gm[2];
      adj_a2.x += g_s;
      qt adj_q_w = Q4(0, 0, 0, 0), adj_r_err = adj_q_w;
      adj_qrot_inv(C.q_w, N, adj_q_w, adj_N, adj_u);
      adj_qmul_a(J.q_off, adj_q_wj, adj_q_w);
      // the axis chain and the decomposition, as k_joint_coords_vjp
      float adj_ang[3] = {0.f, 0.f, 0.f};
      qt adj_q10 = Q4(0, 0, 0, 0), adj_q_1 = adj_q10, adj_q_0 = adj_q10;
      adj_qrot_q(C.q10, V3(0, 0, 1), adj_q10, adj_a2);
      adj_qmul(C.q_1, C.q_0, adj_q_1, adj_q_0, adj_q10);
      adj_q_axis_angle(C.a1, C.ang[1], adj_a1, adj_ang[1], adj_q_1);
      adj_qrot_q(C.q_0, V3(0, 1, 0), adj_q_0, adj_a1);
      adj_q_axis_angle_ang(V3(1, 0, 0), C.ang[0], adj_ang[0], adj_q_0);
      qt adj_q_pc = Q4(0, 0, 0, 0), adj_qa = adj_q_pc;
      quat_decompose_adj(C.q_pc, C.c0, C.c1, C.c2, adj_ang, adj_q_pc);
      adj_qmul_a(J.q_off, adj_qa, adj_q_pc);
      adj_qmul_b(qconj(J.q_off), adj_r_err, adj_qa);
      qt adj_cq = Q4(0, 0, 0, 0);
      adj_qmul(qconj(J.q_wj), B.s.r, adj_cq, own_q, adj_r_err);  // r_err = conj(q_wj) q_c
      adj_q_wj += qconj(adj_cq);
    }
    aM = adj_N;
    adj_cross(B.r, F, adj_r, aF, -adj_N);  // N = M - r x F
    if (J.type != PD_JOINT_FREE) {          // (a FREE joint's r is d: it joins the body's own adjoint below)
      if (J.parent >= 0) {                  // r = (p_p - o0) + R(q_p) p_pj
        par_p += adj_r;
        adj_qrot_q(J.qp, J.p_pj, par_q, adj_r);
      }
      adj_r = V3(0, 0, 0);
    }
    if (J.parent >= 0) adj_qmul_a(J.q_pj, par_q, adj_q_wj);  // q_wj = q_p q_pj
  }
  float *ps = pslot + threadIdx.x * GF_S;
  ps[0] = par_p.x; ps[1] = par_p.y; ps[2] = par_p.z; ps[3] = par_q.x; ps[4] = par_q.y; ps[5] = par_q.z; ps[6] = par_q.w;
  // the ancestor sums: levels from the roots down, a body adds its parent's slot to its own and publishes it
  float *dn = down + threadIdx.x * GF_S;
  gf_put(dn, aF, aM);
  for (int lev = 1; lev <= T.maxd; ++lev) {
    __syncthreads();
    if (L.in_set && T.dep == lev && T.parent >= 0) {
      const float *pp = down + (L.set_l * nb + T.parent) * GF_S;
      aF += ld3(pp); aM += ld3(pp + 3);
      gf_put(dn, aF, aM);
    }
  }
  __syncthreads();  // (pslot; with maxd = 0 the one barrier)
  if (!L.active) return;
  // the body's own share: m_b = t_b + d x f_b, d = (p_b - o0) + R(q_b) com_b
  v3 adj_d = adj_r, adj_f = aF;
  adj_cross(B.d, B.s.v, adj_d, adj_f, aM);
  own_p += adj_d;
  adj_qrot_q(B.s.r, B.J.com, own_q, adj_d);
  for (int k = 0; k < T.nch; ++k) {
    const int c = (int)T.ch[k];
    if (c >= 0 && c < nb) {
      const float *cs = pslot + (L.set_l * nb + c) * GF_S;
      own_p += ld3(cs); own_q += ld4(cs + 3);
    }
  }
  dst[0] = own_p.x; dst[1] = own_p.y; dst[2] = own_p.z;
  dst[3] = own_q.x; dst[4] = own_q.y; dst[5] = own_q.z; dst[6] = own_q.w;
  dst[7] = aM.x; dst[8] = aM.y; dst[9] = aM.z;
  dst[10] = adj_f.x; dst[11] = adj_f.y; dst[12] = adj_f.z;
}

// ---- PD_POSE_BODY_TWIST: the rigid twists of joint rates -- J of the articulation applied to rows (p, q xyzw, r_0..r_5), the exact
// transpose of PD_POSE_GENERALIZED_FORCE in each mode -- and its vector-Jacobian product with respect to poses and rates.  Per joint i,
// on jc_joint's frames and jc_compound's angles and axes, r_i = the joint's anchor - o0 as gf_load forms it:
//   REVOLUTE  w_i = (R_wj axis) r_0                   u_i = 0             anchor p_wj
//   COMPOUND  w_i = R_wj R_off sum_k a_k rho_k        u_i = 0             anchor p_wj;  mode 1 (generalized): rho = r; mode 0 (measured):
//             rho = G^-1 r, the Gram solve (rho_1 = r_1, (rho_0, rho_2) = ((r_0 - s r_2), (r_2 - s r_0)) / (1 - s^2))
//   FREE      w_i = R_wj r_0..2                       u_i = R_wj r_3..5   anchor x_i;   FIXED: nothing
//   w_b = W_b = sum w_i,  v_b = C_b + W_b x d_b,  C_b = sum (u_i - w_i x r_i), the sums over b and its ancestors, d_b = x_b - o0
// Mapping and sweeps are the generalised force's, mirrored: forward the ancestor sum (gf_down), VJP the ancestor sum of w (adj d needs
// W_b), then subtree sums of (adj C, adj W) = (g_v, g_w + d x g_v) through gf_up, the joint's adjoint -- the rate adjoints are the
// generalised force's projections --, and the parent-side pose adjoint handed over.  No atomics; every float has one writing lane.
// Ancestor sums of (a, b): levels from the roots down, a body adds its parent's slot to its own and publishes it -- the loop of
// k_generalized_force_vjp, which keeps its own copy (calling this from there changes that kernel's instruction stream).
__device__ __forceinline__ void gf_down(float *down, const GfTree &T, const SetLane &L, int nb, v3 &a, v3 &b) {
  float *dn = down + threadIdx.x * GF_S;
  gf_put(dn, a, b);
  for (int lev = 1; lev <= T.maxd; ++lev) {
    __syncthreads();
    if (L.in_set && T.dep == lev && T.parent >= 0) {
      const float *pp = down + (L.set_l * nb + T.parent) * GF_S;
      a += ld3(pp); b += ld3(pp + 3);
      gf_put(dn, a, b);
    }
  }
}
struct BtJoint { v3 w, u, e; JcCompound C; float rho[3]; };  // e: the COMPOUND rate in the offset frame, w = R(q_w) e
__device__ __forceinline__ void bt_joint(const GfBody &B, bool generalized, BtJoint &Q) {
  const JcJoint &J = B.J;
  Q.w = V3(0, 0, 0); Q.u = Q.w; Q.e = Q.w;
  if (J.type == PD_JOINT_FREE) {
    Q.w = qrot(J.q_wj, B.s.w); Q.u = qrot(J.q_wj, B.s.v);
  } else if (J.type == PD_JOINT_REVOLUTE) {
    Q.w = qrot(J.q_wj, J.axis) * B.s.w.x;
  } else if (J.type == PD_JOINT_COMPOUND) {
    jc_compound(J, false, Q.C);
    const float s = Q.C.s;
    Q.rho[0] = B.s.w.x; Q.rho[1] = B.s.w.y; Q.rho[2] = B.s.w.z;
    if (!generalized) {
      const float id = 1.0f / (1.0f - s * s);
      Q.rho[0] = (B.s.w.x - s * B.s.w.z) * id; Q.rho[2] = (B.s.w.z - s * B.s.w.x) * id;
    }
    Q.e = V3(Q.rho[0], 0, 0) + Q.C.a1 * Q.rho[1] + Q.C.a2 * Q.rho[2];
    Q.w = qrot(Q.C.q_w, Q.e);
  }
}

__global__ __launch_bounds__(256) void k_body_twist_fwd(int nsets, int nb, const float *__restrict__ tab, const float *__restrict__ rows,
                                                        float *__restrict__ out) {
  __shared__ float down[256 * GF_S];
  __shared__ int s_anc[2][256], s_dep[2][256], s_max[4];
  const SetLane L = set_lane(nsets, nb);
  float *o = out + ((size_t)L.set * nb + L.body) * 6;  // (formed, not touched, by an inactive lane)
  if ((int)tab[0] != nb) {  // not this call's table (the same for every lane of the launch: no barrier is skipped by some)
    if (L.active)
      for (int k = 0; k < 6; ++k) o[k] = 0.0f;
    return;
  }
  const bool generalized = tab[3] != 0.0f;
  const GfTree T = gf_tree(tab, nb, L, s_anc, s_dep, s_max);
  GfBody B;
  v3 W = V3(0, 0, 0), C = W;
  if (L.active) {
    gf_load(tab, nb, L.body, rows + (size_t)L.set * nb * PD_ADJ, B);
    BtJoint Q;
    bt_joint(B, generalized, Q);
    W = Q.w; C = Q.u - cross(Q.w, B.r);
  }
  gf_down(down, T, L, nb, W, C);
  if (!L.active) return;
  const v3 v = C + cross(W, B.d);
  o[0] = W.x; o[1] = W.y; o[2] = W.z; o[3] = v.x; o[4] = v.y; o[5] = v.z;
}

// g_b [n][13]: the raw partials of <g_out, out> with respect to (p, q, r_0..r_5) of every body; a slot past the joint's dofs gets zero.
__global__ __launch_bounds__(256) void k_body_twist_vjp(int nsets, int nb, const float *__restrict__ tab, const float *__restrict__ rows,
                                                        const float *__restrict__ g_out, float *__restrict__ g_b) {
  __shared__ float slot[256 * GF_S], down[256 * GF_S], pslot[256 * GF_S];  // subtree sums / ancestor sums / the parent-side pose adjoint
  __shared__ int s_anc[2][256], s_dep[2][256], s_max[4];
  const SetLane L = set_lane(nsets, nb);
  float *dst = g_b + ((size_t)L.set * nb + L.body) * PD_ADJ;  // (formed, not touched, by an inactive lane)
  if ((int)tab[0] != nb) {
    if (L.active)
      for (int k = 0; k < PD_ADJ; ++k) dst[k] = 0.0f;
    return;
  }
  const bool generalized = tab[3] != 0.0f;
  const GfTree T = gf_tree(tab, nb, L, s_anc, s_dep, s_max);
  GfBody B;
  BtJoint Q;
  v3 W = V3(0, 0, 0), C = W;
  if (L.active) {
    gf_load(tab, nb, L.body, rows + (size_t)L.set * nb * PD_ADJ, B);
    bt_joint(B, generalized, Q);
    W = Q.w; C = Q.u - cross(Q.w, B.r);
  }
  gf_down(down, T, L, nb, W, C);
  // the body's own share: w_b = W, v_b = C + W x d
  v3 F = V3(0, 0, 0), M = F, adj_d = F;
  if (L.active) {
    const float *g = g_out + ((size_t)L.set * nb + L.body) * 6;
    F = ld3(g + 3); M = ld3(g);
    adj_cross(W, B.d, M, adj_d, F);
  }
  gf_up(slot, T, L, nb, F, M);  // (adj C, adj W) of the joint's subtree
  v3 own_p = V3(0, 0, 0), par_p = own_p;
  qt own_q = Q4(0, 0, 0, 0), par_q = own_q;
  float gr[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (L.active) {
    const JcJoint &J = B.J;
    const v3 N = M - cross(B.r, F);  // adj w_i: c_i = u_i - w_i x r_i
    v3 adj_r = cross(Q.w, F);
    qt adj_q_wj = Q4(0, 0, 0, 0);
    if (J.type == PD_JOINT_FREE) {
      const v3 a = qrot_inv(J.q_wj, N), l = qrot_inv(J.q_wj, F);
      gr[0] = a.x; gr[1] = a.y; gr[2] = a.z; gr[3] = l.x; gr[4] = l.y; gr[5] = l.z;
      adj_qrot_q(J.q_wj, B.s.w, adj_q_wj, N);
      adj_qrot_q(J.q_wj, B.s.v, adj_q_wj, F);
    } else if (J.type == PD_JOINT_REVOLUTE) {
      gr[0] = dot(qrot(J.q_wj, J.axis), N);
      adj_qrot_q(J.q_wj, J.axis, adj_q_wj, N * B.s.w.x);
    } else if (J.type == PD_JOINT_COMPOUND) {
      const JcCompound &K = Q.C;
      const v3 u = qrot_inv(K.q_w, N);  // adj e
      float gm[3] = {u.x, dot(K.a1, u), dot(K.a2, u)}, g_s = 0.0f;  // adj rho
      gr[0] = gm[0]; gr[1] = gm[1]; gr[2] = gm[2];
      if (!generalized) {  // rho_0 = (r_0 - s r_2) id, rho_2 = (r_2 - s r_0) id, id = 1 / (1 - s^2)
        const float id = 1.0f / (1.0f - K.s * K.s);
        g_s = (gm[0] * (2.0f * K.s * Q.rho[0] - B.s.w.z) + gm[2] * (2.0f * K.s * Q.rho[2] - B.s.w.x)) * id;
        gr[0] = (gm[0] - K.s * gm[2]) * id;
        gr[2] = (gm[2] - K.s * gm[0]) * id;
      }
      v3 adj_a1 = u * Q.rho[1], adj_a2 = u * Q.rho[2];
      adj_a2.x += g_s;
      qt adj_q_w = Q4(0, 0, 0, 0), adj_r_err = adj_q_w;
      adj_qrot_q(K.q_w, Q.e, adj_q_w, N);
      adj_qmul_a(J.q_off, adj_q_wj, adj_q_w);
      // the axis chain and the decomposition, as k_generalized_force_vjp
      float adj_ang[3] = {0.f, 0.f, 0.f};
      qt adj_q10 = Q4(0, 0, 0, 0), adj_q_1 = adj_q10, adj_q_0 = adj_q10;
      adj_qrot_q(K.q10, V3(0, 0, 1), adj_q10, adj_a2);
      adj_qmul(K.q_1, K.q_0, adj_q_1, adj_q_0, adj_q10);
      adj_q_axis_angle(K.a1, K.ang[1], adj_a1, adj_ang[1], adj_q_1);
      adj_qrot_q(K.q_0, V3(0, 1, 0), adj_q_0, adj_a1);
      adj_q_axis_angle_ang(V3(1, 0, 0), K.ang[0], adj_ang[0], adj_q_0);
      qt adj_q_pc = Q4(0, 0, 0, 0), adj_qa = adj_q_pc;
      quat_decompose_adj(K.q_pc, K.c0, K.c1, K.c2, adj_ang, adj_q_pc);
      adj_qmul_a(J.q_off, adj_qa, adj_q_pc);
      adj_qmul_b(qconj(J.q_off), adj_r_err, adj_qa);
      qt adj_cq = Q4(0, 0, 0, 0);
      adj_qmul(qconj(J.q_wj), B.s.r, adj_cq, own_q, adj_r_err);  // r_err = conj(q_wj) q_c
      adj_q_wj += qconj(adj_cq);
    }
    if (J.type == PD_JOINT_FREE) adj_d += adj_r;  // (a FREE joint's r is d)
    else if (J.parent >= 0) {                     // r = (p_p - o0) + R(q_p) p_pj
      par_p += adj_r;
      adj_qrot_q(J.qp, J.p_pj, par_q, adj_r);
    }
    if (J.parent >= 0) adj_qmul_a(J.q_pj, par_q, adj_q_wj);  // q_wj = q_p q_pj
    own_p += adj_d;  // d = (p_b - o0) + R(q_b) com_b
    adj_qrot_q(B.s.r, J.com, own_q, adj_d);
  }
  float *ps = pslot + threadIdx.x * GF_S;
  ps[0] = par_p.x; ps[1] = par_p.y; ps[2] = par_p.z; ps[3] = par_q.x; ps[4] = par_q.y; ps[5] = par_q.z; ps[6] = par_q.w;
  __syncthreads();
  if (!L.active) return;
  for (int k = 0; k < T.nch; ++k) {
    const int c = (int)T.ch[k];
    if (c >= 0 && c < nb) {
      const float *cs = pslot + (L.set_l * nb + c) * GF_S;
      own_p += ld3(cs); own_q += ld4(cs + 3);
    }
  }
  dst[0] = own_p.x; dst[1] = own_p.y; dst[2] = own_p.z;
  dst[3] = own_q.x; dst[4] = own_q.y; dst[5] = own_q.z; dst[6] = own_q.w;
#pragma unroll
  for (int k = 0; k < 6; ++k) dst[7 + k] = gr[k];
}

// ---- PD_POSE_BODY_ACCEL: the accelerations of the bodies of a state -- J qdd + Jdot qd of the articulation -- from rows
// (p, q xyzw, w, v, s_0..s_5): a state row and the time derivatives of the rate slots of the body's joint, and its vector-Jacobian
// product with respect to the whole row.  State-based: every velocity-dependent term comes from the row's own twist and its parent's.
// Per joint i with parent pi (w_pi = v_pi = 0 and a constant frame without one), on jc_joint's frames and jc_compound's angles and axes:
//   every joint  om_i = w_i - w_pi (jc_joint's w_err);  omd_i = (the joint's term) + w_pi x om_i
//   REVOLUTE     term (R_wj axis) s_0                       ud_i = 0     anchor o_i = p_wj,  od_i = v_pi + w_pi x (p_wj - x_pi)
//   COMPOUND     rho = G^-1 m of jc_compound (always the Gram solve);  mode 1: rhod = s_0..2;  mode 0: rhod = G^-1 (s_0 - sd rho_2, s_1,
//                s_2 - sd rho_0), sd = rho_1 a_0 . (a_1 x a_2);  term sum_k ah_k rhod_k + sum_{k<l} rho_k rho_l ah_k x ah_l, ah_k = R_wj R_off a_k
//                ud_i = 0, anchor as REVOLUTE
//   FREE         u_i = v_i - v_pi - w_pi x (x_i - x_pi);  term R_wj s_0..2;  ud_i = R_wj s_3..5 + w_pi x u_i;  o_i = x_i, od_i = v_i
//   FIXED        no term, anchor as REVOLUTE
//   e_i = ud_i - omd_i x (o_i - o0) - om_i x od_i
//   alpha_b = sum omd_i,  a_b = sum e_i + alpha_b x d_b + w_b x v_b,  the sums over b and its ancestors, d_b = x_b - o0
// Mapping and sweeps are the body twist's: forward one ancestor sum (gf_down); VJP the ancestor sum again (adj d needs alpha_b), subtree
// sums of (adj E, adj alpha) = (g_a, g_alpha + d x g_a) through gf_up, the joint's adjoint -- the s adjoints are the body twist's
// projections, the rho adjoints flow into w_i - w_pi through the m_k --, and the parent-side adjoint, now a whole state row (pose AND
// twist of the parent enter), handed over in an LDS slot of 13 floats as k_joint_coords_vjp does.  No atomics; one writing lane per float.
enum { BA_ROW = 19 };
struct BaBody { BodyState s; JcJoint J; v3 d, ro, od, l, com_p, sa, sv; };  // (sa, sv) = s_0..2, s_3..5; ro = o_i - o0; l = p_wj - x_pi (FREE: x_i - x_pi), 0 without a parent
__device__ __forceinline__ void ba_load(const float *tab, int nb, int body, const float *set_rows, BaBody &B) {
  const v3 o0 = ld3(set_rows);
  const float *r = set_rows + (size_t)body * BA_ROW;
  B.s = load_row<BA_ROW>(set_rows, (size_t)body);
  B.sa = ld3(r + 13); B.sv = ld3(r + 16);
  B.J = jc_joint<BA_ROW>(tab, nb, (int)tab[1], (int)tab[2], body, B.s, set_rows);
  const JcJoint &J = B.J;
  B.d = (B.s.p - o0) + qrot(B.s.r, J.com);
  const bool fr = J.type == PD_JOINT_FREE, hp = J.parent >= 0;
  v3 com_p = V3(0, 0, 0);
  if (hp) com_p = ld3(tab + JC_HEAD + JC_BODY * J.parent + 18);
  // (without a parent jc_joint leaves pp = 0, qp = 1, w_p = v_p = 0: the anchor is p_pj - o0 and od vanishes by the same lines)
  v3 l = fr ? B.d - ((J.pp - o0) + qrot(J.qp, com_p)) : qrot(J.qp, J.p_pj - com_p);
  if (!hp) l = V3(0, 0, 0);
  B.com_p = com_p; B.l = l;
  B.ro = fr ? B.d : (J.pp - o0) + qrot(J.qp, J.p_pj);
  B.od = fr ? B.s.v : J.v_p + cross(J.w_p, l);
}
// omd_i, ud_i and what the adjoint needs of them.  COMPOUND: eps = sum_k a_k rhod_k in the offset frame, ah_k = R_wj R_off a_k (the
// products ah_k x ah_l are formed from the ROTATED axes, as the definition states them: the raw partials with respect to a quaternion
// that leaves the unit sphere see the difference to R (a_k x a_l)), t = the right-hand side of the mode-0 Gram solve,
// sd = d(a_0 . a_2) / dt, trip = a_0 . (a_1 x a_2)
struct BaJoint { v3 omd, ud, u, eps, ah0, ah1, ah2; JcCompound C; v3 rho, rhod, t; float sd, trip; };
__device__ __forceinline__ void ba_joint(const BaBody &B, bool generalized, BaJoint &Q) {
  const JcJoint &J = B.J;
  const v3 bias = cross(J.w_p, J.w_err);
  Q.omd = bias; Q.ud = V3(0, 0, 0); Q.u = Q.ud; Q.eps = Q.ud;
  if (J.type == PD_JOINT_FREE) {
    Q.u = (B.s.v - J.v_p) - cross(J.w_p, B.l);
    Q.omd = qrot(J.q_wj, B.sa) + bias;
    Q.ud = qrot(J.q_wj, B.sv) + cross(J.w_p, Q.u);
  } else if (J.type == PD_JOINT_REVOLUTE) {
    Q.omd = qrot(J.q_wj, J.axis) * B.sa.x + bias;
  } else if (J.type == PD_JOINT_COMPOUND) {
    JcCompound &C = Q.C;
    jc_compound(J, false, C);
    C.id = 1.0f / (1.0f - C.s * C.s);  // rho = G^-1 m in either mode
    Q.rho = V3((C.m[0] - C.s * C.m[2]) * C.id, C.m[1], (C.m[2] - C.s * C.m[0]) * C.id);
    Q.rhod = B.sa; Q.t = B.sa;
    Q.trip = cross(C.a1, C.a2).x; Q.sd = Q.rho.y * Q.trip;
    if (!generalized) {
      Q.t.x = B.sa.x - Q.sd * Q.rho.z; Q.t.z = B.sa.z - Q.sd * Q.rho.x;
      Q.rhod.x = (Q.t.x - C.s * Q.t.z) * C.id; Q.rhod.z = (Q.t.z - C.s * Q.t.x) * C.id;
    }
    Q.eps = V3(Q.rhod.x, 0, 0) + C.a1 * Q.rhod.y + C.a2 * Q.rhod.z;
    Q.ah0 = qrot(C.q_w, V3(1, 0, 0)); Q.ah1 = qrot(C.q_w, C.a1); Q.ah2 = qrot(C.q_w, C.a2);
    Q.omd = qrot(C.q_w, Q.eps) + bias + cross(Q.ah0, Q.ah1) * (Q.rho.x * Q.rho.y) + cross(Q.ah0, Q.ah2) * (Q.rho.x * Q.rho.z) +
            cross(Q.ah1, Q.ah2) * (Q.rho.y * Q.rho.z);
  }
}

__global__ __launch_bounds__(256) void k_body_accel_fwd(int nsets, int nb, const float *__restrict__ tab, const float *__restrict__ rows,
                                                        float *__restrict__ out) {
  __shared__ float down[256 * GF_S];
  __shared__ int s_anc[2][256], s_dep[2][256], s_max[4];
  const SetLane L = set_lane(nsets, nb);
  float *o = out + ((size_t)L.set * nb + L.body) * 6;  // (formed, not touched, by an inactive lane)
  if ((int)tab[0] != nb) {  // not this call's table (the same for every lane of the launch: no barrier is skipped by some)
    if (L.active)
      for (int k = 0; k < 6; ++k) o[k] = 0.0f;
    return;
  }
  const bool generalized = tab[3] != 0.0f;
  const GfTree T = gf_tree(tab, nb, L, s_anc, s_dep, s_max);
  BaBody B;
  v3 A = V3(0, 0, 0), E = A;
  if (L.active) {
    ba_load(tab, nb, L.body, rows + (size_t)L.set * nb * BA_ROW, B);
    BaJoint Q;
    ba_joint(B, generalized, Q);
    A = Q.omd; E = Q.ud - cross(Q.omd, B.ro) - cross(B.J.w_err, B.od);
  }
  gf_down(down, T, L, nb, A, E);
  if (!L.active) return;
  const v3 a = E + cross(A, B.d) + cross(B.s.w, B.s.v);
  o[0] = A.x; o[1] = A.y; o[2] = A.z; o[3] = a.x; o[4] = a.y; o[5] = a.z;
}

// g_b [n][19]: the raw partials of <g_out, out> with respect to (p, q, w, v, s_0..s_5) of every body; a slot past the joint's dofs gets zero.
__global__ __launch_bounds__(256) void k_body_accel_vjp(int nsets, int nb, const float *__restrict__ tab, const float *__restrict__ rows,
                                                        const float *__restrict__ g_out, float *__restrict__ g_b) {
  __shared__ float slot[256 * GF_S], down[256 * GF_S], pslot[256 * PD_ADJ];  // subtree sums / ancestor sums / the parent-side adjoint (odd strides)
  __shared__ int s_anc[2][256], s_dep[2][256], s_max[4];
  const SetLane L = set_lane(nsets, nb);
  float *dst = g_b + ((size_t)L.set * nb + L.body) * BA_ROW;  // (formed, not touched, by an inactive lane)
  if ((int)tab[0] != nb) {
    if (L.active)
      for (int k = 0; k < BA_ROW; ++k) dst[k] = 0.0f;
    return;
  }
  const bool generalized = tab[3] != 0.0f;
  const GfTree T = gf_tree(tab, nb, L, s_anc, s_dep, s_max);
  BaBody B;
  BaJoint Q;
  v3 A = V3(0, 0, 0), E = A;
  if (L.active) {
    ba_load(tab, nb, L.body, rows + (size_t)L.set * nb * BA_ROW, B);
    ba_joint(B, generalized, Q);
    A = Q.omd; E = Q.ud - cross(Q.omd, B.ro) - cross(B.J.w_err, B.od);
  }
  gf_down(down, T, L, nb, A, E);
  // the body's own share: alpha_b = A, a_b = E + A x d + w x v
  BodyAdj own = adj_zero(), par = adj_zero();
  v3 F = V3(0, 0, 0), M = F, adj_d = F;
  if (L.active) {
    const float *g = g_out + ((size_t)L.set * nb + L.body) * 6;
    F = ld3(g + 3); M = ld3(g);
    adj_cross(A, B.d, M, adj_d, F);
    adj_cross(B.s.w, B.s.v, own.w, own.v, F);
  }
  gf_up(slot, T, L, nb, F, M);  // (adj e_i, adj omd_i before e_i's share) of the joint's subtree
  float gs[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (L.active) {
    const JcJoint &J = B.J;
    const bool has_par = J.parent >= 0;
    // e_i = ud_i - omd_i x ro - om_i x od_i
    v3 N = M, adj_ro = V3(0, 0, 0), adj_om = adj_ro, adj_od = adj_ro, adj_wp = adj_ro, adj_l = adj_ro;
    adj_cross(Q.omd, B.ro, N, adj_ro, -F);
    adj_cross(J.w_err, B.od, adj_om, adj_od, -F);
    adj_cross(J.w_p, J.w_err, adj_wp, adj_om, N);  // omd_i = term + w_pi x om_i
    qt adj_q_wj = Q4(0, 0, 0, 0);
    if (J.type == PD_JOINT_FREE) {
      const v3 a = qrot_inv(J.q_wj, N), l = qrot_inv(J.q_wj, F);
      gs[0] = a.x; gs[1] = a.y; gs[2] = a.z; gs[3] = l.x; gs[4] = l.y; gs[5] = l.z;
      adj_qrot_q(J.q_wj, B.sa, adj_q_wj, N);
      adj_qrot_q(J.q_wj, B.sv, adj_q_wj, F);
      v3 adj_u = V3(0, 0, 0);
      adj_cross(J.w_p, Q.u, adj_wp, adj_u, F);  // ud_i = R_wj s_3..5 + w_pi x u_i
      own.v += adj_u; par.v -= adj_u;           // u_i = v_i - v_pi - w_pi x l
      adj_cross(J.w_p, B.l, adj_wp, adj_l, -adj_u);
      own.v += adj_od;                          // od_i = v_i, ro = d
      adj_d += adj_ro;
      if (has_par) {                            // l = d - ((p_pi - o0) + R(q_pi) com_pi)
        adj_d += adj_l;
        par.p -= adj_l;
        adj_qrot_q(J.qp, B.com_p, par.r, -adj_l);
      }
    } else {
      if (has_par) {  // ro = (p_pi - o0) + R(q_pi) p_pj, od_i = v_pi + w_pi x l, l = R(q_pi) (p_pj - com_pi)
        par.p += adj_ro;
        adj_qrot_q(J.qp, J.p_pj, par.r, adj_ro);
        par.v += adj_od;
        adj_cross(J.w_p, B.l, adj_wp, adj_l, adj_od);
        adj_qrot_q(J.qp, J.p_pj - B.com_p, par.r, adj_l);
      }
      if (J.type == PD_JOINT_REVOLUTE) {
        gs[0] = dot(qrot(J.q_wj, J.axis), N);
        adj_qrot_q(J.q_wj, J.axis, adj_q_wj, N * B.sa.x);
      } else if (J.type == PD_JOINT_COMPOUND) {
        const JcCompound &K = Q.C;
        const v3 ae = qrot_inv(K.q_w, N);  // adj eps
        float grd[3] = {ae.x, dot(K.a1, ae), dot(K.a2, ae)}, g_s = 0.0f;  // adj rhod
        const float p01 = dot(cross(Q.ah0, Q.ah1), N), p02 = dot(cross(Q.ah0, Q.ah2), N), p12 = dot(cross(Q.ah1, Q.ah2), N);
        float grho[3] = {Q.rho.y * p01 + Q.rho.z * p02, Q.rho.x * p01 + Q.rho.z * p12, Q.rho.x * p02 + Q.rho.y * p12};
        v3 adj_a1 = ae * Q.rhod.y, adj_a2 = ae * Q.rhod.z, adj_c12 = V3(0, 0, 0);
        qt adj_q_w = Q4(0, 0, 0, 0), adj_r_err = adj_q_w;
        {  // the products of the rotated axes, ah_k = R(q_w) a_k
          v3 adj_h0 = V3(0, 0, 0), adj_h1 = adj_h0, adj_h2 = adj_h0;
          adj_cross(Q.ah0, Q.ah1, adj_h0, adj_h1, N * (Q.rho.x * Q.rho.y));
          adj_cross(Q.ah0, Q.ah2, adj_h0, adj_h2, N * (Q.rho.x * Q.rho.z));
          adj_cross(Q.ah1, Q.ah2, adj_h1, adj_h2, N * (Q.rho.y * Q.rho.z));
          adj_qrot_q(K.q_w, V3(1, 0, 0), adj_q_w, adj_h0);
          adj_qrot(K.q_w, K.a1, adj_q_w, adj_a1, adj_h1);
          adj_qrot(K.q_w, K.a2, adj_q_w, adj_a2, adj_h2);
        }
        gs[0] = grd[0]; gs[1] = grd[1]; gs[2] = grd[2];
        if (!generalized) {  // rhod_0 = (t_0 - s t_2) id, rhod_2 = (t_2 - s t_0) id; t_0 = s_0 - sd rho_2, t_2 = s_2 - sd rho_0; sd = rho_1 trip
          g_s = (grd[0] * (2.0f * K.s * Q.rhod.x - Q.t.z) + grd[2] * (2.0f * K.s * Q.rhod.z - Q.t.x)) * K.id;
          gs[0] = (grd[0] - K.s * grd[2]) * K.id;
          gs[2] = (grd[2] - K.s * grd[0]) * K.id;
          const float g_sd = -(gs[0] * Q.rho.z + gs[2] * Q.rho.x);
          grho[2] -= gs[0] * Q.sd; grho[0] -= gs[2] * Q.sd;
          grho[1] += g_sd * Q.trip;
          adj_c12.x += g_sd * Q.rho.y;
        }
        adj_cross(K.a1, K.a2, adj_a1, adj_a2, adj_c12);
        // rho = G^-1 m, m_k = a_k . u, u = R_w^T om_i
        g_s += (grho[0] * (2.0f * K.s * Q.rho.x - K.m[2]) + grho[2] * (2.0f * K.s * Q.rho.z - K.m[0])) * K.id;
        const float gm0 = (grho[0] - K.s * grho[2]) * K.id, gm2 = (grho[2] - K.s * grho[0]) * K.id, gm1 = grho[1];
        const v3 adj_u = V3(gm0, 0, 0) + K.a1 * gm1 + K.a2 * gm2;
        adj_a1 += K.u * gm1; adj_a2 += K.u * gm2;
        adj_a2.x += g_s;
        adj_qrot_q(K.q_w, Q.eps, adj_q_w, N);
        adj_qrot_inv(K.q_w, J.w_err, adj_q_w, adj_om, adj_u);
        adj_qmul_a(J.q_off, adj_q_wj, adj_q_w);
        // the axis chain and the decomposition, as k_body_twist_vjp
        float adj_ang[3] = {0.f, 0.f, 0.f};
        qt adj_q10 = Q4(0, 0, 0, 0), adj_q_1 = adj_q10, adj_q_0 = adj_q10;
        adj_qrot_q(K.q10, V3(0, 0, 1), adj_q10, adj_a2);
        adj_qmul(K.q_1, K.q_0, adj_q_1, adj_q_0, adj_q10);
        adj_q_axis_angle(K.a1, K.ang[1], adj_a1, adj_ang[1], adj_q_1);
        adj_qrot_q(K.q_0, V3(0, 1, 0), adj_q_0, adj_a1);
        adj_q_axis_angle_ang(V3(1, 0, 0), K.ang[0], adj_ang[0], adj_q_0);
        qt adj_q_pc = Q4(0, 0, 0, 0), adj_qa = adj_q_pc;
        quat_decompose_adj(K.q_pc, K.c0, K.c1, K.c2, adj_ang, adj_q_pc);
        adj_qmul_a(J.q_off, adj_qa, adj_q_pc);
        adj_qmul_b(qconj(J.q_off), adj_r_err, adj_qa);
        qt adj_cq = Q4(0, 0, 0, 0);
        adj_qmul(qconj(J.q_wj), B.s.r, adj_cq, own.r, adj_r_err);  // r_err = conj(q_wj) q_c
        adj_q_wj += qconj(adj_cq);
      }
    }
    own.w += adj_om;  // om_i = w_i - w_pi
    if (has_par) {
      par.w += adj_wp - adj_om;
      adj_qmul_a(J.q_pj, par.r, adj_q_wj);  // q_wj = q_pi q_pj
    }
    own.p += adj_d;  // d = (p_b - o0) + R(q_b) com_b
    adj_qrot_q(B.s.r, J.com, own.r, adj_d);
  }
  adj_store(pslot + threadIdx.x * PD_ADJ, par);
  __syncthreads();
  if (!L.active) return;
  for (int k = 0; k < T.nch; ++k) {
    const int c = (int)T.ch[k];
    if (c >= 0 && c < nb) adj_add_from(own, pslot + (L.set_l * nb + c) * PD_ADJ);
  }
  float o[PD_ADJ];
  adj_store(o, own);
#pragma unroll
  for (int k = 0; k < PD_ADJ; ++k) dst[k] = o[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) dst[PD_ADJ + k] = gs[k];
}

// ---- PD_POSE_MASS_INVERSE: H^-1 applied to a joint-space vector, H = sum_b J_b^T diag(R_b I_b R_b^T, m_b) J_b the mass matrix of the
// articulation (J = PD_POSE_BODY_TWIST's Jacobian in the table's mode), by the articulated-body recursion, from rows
// (p, q xyzw, m, I row-major, r_0..r_5): the pose, the body's mass and body-frame inertia about its centre of mass (its symmetric part
// enters) and the joint-space force entries of the body's joint in the body twist's slot layout -> the solution in the same slots.
// Everything in world axes about o0 = the origin of the set's body 0, spatial vectors (angular, linear at o0): children's quantities add
// without a transform, like gf_up's (F, M).  Per body, d = x_b - o0, Ibar = R sym(I) R^T, r_i = the joint's anchor - o0 as gf_load forms it:
//   spatial inertia  [[Ibar - m [d]x[d]x, m [d]x], [-m [d]x, m 1]]   (symmetric: 21 floats, mi_ix)
//   motion subspace  REVOLUTE (ah, -ah x r_i);  COMPOUND three such columns from Ah = R_wj R_off (a_0 a_1 a_2) (mode 1) or Ah G^-1 (mode 0,
//                    as bt_joint reads its rates);  FREE (R_wj e_k, -R_wj e_k x d_b) and (0, R_wj e_k);  FIXED none
// Up, deepest level first:  IA = I_b + sum Ia_c, pA = sum pa_c (the table's child order), U = IA S, D = S^T U = L diag(dd) L^T,
//   W = L^-1 U^T, z = L^-1 (r_b - S^T pA);  the body hands up Ia = IA - W^T dd^-1 W and pa = pA + W^T dd^-1 z through an LDS slot of 27
//   floats (odd stride: distinct banks); behind a 6-dof joint Ia is exactly 0, not the rounding residue; a body without a dof hands
//   IA, pA up unchanged.  Down, from the roots:  x_b = L^-T dd^-1 (z - W a_pi),  a_b = a_pi + S x_b, six floats per body.
// D (1x1, 3x3, 6x6) is never inverted: the LDL^T factor is applied by substitution (the explicit inverse loses 6e-3 of max |x| on the
// human in fp32).  A pivot that is not positive gives inf / NaN, as a singular H does in a dense solve; not guarded.
// Precision: rows, frames, motion subspaces, the 27 + 6 floats handed over and the kept factor are fp32; the body's own spatial inertia,
// the sums over children, the factor and the substitutions are evaluated in double (an fp32 recursion is 1e-5 .. 4e-5 off on the human,
// almost all of it from the recursion's own roundings; this form 2e-6: DESIGN.md section 8).
// The factor of every joint size is the same unrolled template: every array index is a constant, nothing is indexed by the dof count.
// Mapping: a lane per body, whole state sets per workgroup (set_lane), depths from gf_tree; every barrier in workgroup-uniform control
// flow (trip counts are table data); no atomics, one writing lane per float.  A table of another nb: zeros, no row of it is read.
// The op is self-adjoint in its slots (H is symmetric); its gradient is composed on the host side (include/ppr_diffphys.h): no VJP kernel.
enum { MI_ROW = 23, MI_S = 27 };
__device__ __forceinline__ constexpr int mi_ix(int i, int j) {  // the upper triangle of a symmetric 6 x 6, row by row
  return i <= j ? i * 6 - i * (i - 1) / 2 + (j - i) : j * 6 - j * (j - 1) / 2 + (i - j);
}
__device__ __forceinline__ constexpr int mi_lx(int i, int j) { return i * (i - 1) / 2 + j; }  // the strict lower triangle, j < i
struct MiJoint { float S[36], W[36], L[15], di[6], z[6]; };  // column k of S and row k of W at [6 k ..]; di = 1 / the pivots dd
__device__ __forceinline__ void mi_col(float *c, v3 w, v3 l) { c[0] = w.x; c[1] = w.y; c[2] = w.z; c[3] = l.x; c[4] = l.y; c[5] = l.z; }
// The joint's factor from (IA, pA) and its force entries r; (IA, pA) leave as what the body hands up.  The arithmetic is double, what is
// kept (Q) and handed over is float: H of a long or branched chain is ill-conditioned (human: 4e4), and the roundings of an fp32
// recursion -- not those of its fp32 inputs -- are what the solution loses digits to (measured: DESIGN.md section 8).
template <int K>
__device__ __forceinline__ void mi_factor(double *IA, double *pA, const float *r, MiJoint &Q) {
  double W[6 * K], L[K * (K - 1) / 2 + 1], dd[K], di[K], z[K];  // W starts as U = IA S and is reduced in place
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double t = IA[mi_ix(i, 0)] * (double)Q.S[6 * k];
#pragma unroll
      for (int j = 1; j < 6; ++j) t += IA[mi_ix(i, j)] * (double)Q.S[6 * k + j];
      W[6 * k + i] = t;
    }
#pragma unroll
  for (int j = 0; j < K; ++j) {  // D(i, j) = S_i . U_j, formed where it is used (U_j is still whole: rows are reduced below)
    double t = 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) t += (double)Q.S[6 * j + e] * W[6 * j + e];
#pragma unroll
    for (int p = 0; p < j; ++p) t -= L[mi_lx(j, p)] * L[mi_lx(j, p)] * dd[p];
    dd[j] = t;
    di[j] = 1.0 / t;
#pragma unroll
    for (int i = j + 1; i < K; ++i) {
      double u = 0.0;
#pragma unroll
      for (int e = 0; e < 6; ++e) u += (double)Q.S[6 * i + e] * W[6 * j + e];
#pragma unroll
      for (int p = 0; p < j; ++p) u -= L[mi_lx(i, p)] * L[mi_lx(j, p)] * dd[p];
      L[mi_lx(i, j)] = u * di[j];
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double zk = (double)r[k];
#pragma unroll
    for (int e = 0; e < 6; ++e) zk -= (double)Q.S[6 * k + e] * pA[e];
#pragma unroll
    for (int p = 0; p < k; ++p) zk -= L[mi_lx(k, p)] * z[p];
    z[k] = zk;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double w = W[6 * k + i];
#pragma unroll
      for (int p = 0; p < k; ++p) w -= L[mi_lx(k, p)] * W[6 * p + i];
      W[6 * k + i] = w;
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double zd = z[k] * di[k];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      pA[i] += W[6 * k + i] * zd;
      const double wd = W[6 * k + i] * di[k];
#pragma unroll
      for (int j = i; j < 6; ++j) IA[mi_ix(i, j)] -= wd * W[6 * k + j];
    }
  }
  if constexpr (K == 6) {
#pragma unroll
    for (int e = 0; e < 21; ++e) IA[e] = 0.0;
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    Q.di[k] = (float)di[k]; Q.z[k] = (float)z[k];
#pragma unroll
    for (int i = 0; i < 6; ++i) Q.W[6 * k + i] = (float)W[6 * k + i];
#pragma unroll
    for (int p = 0; p < k; ++p) Q.L[mi_lx(k, p)] = (float)L[mi_lx(k, p)];
  }
}
// a: the parent's acceleration in, the body's out; x: the joint's solution.  Double arithmetic on the kept floats.
template <int K>
__device__ __forceinline__ void mi_solve(const MiJoint &Q, double *a, double *x) {
#pragma unroll
  for (int k = K - 1; k >= 0; --k) {
    double t = (double)Q.z[k];
#pragma unroll
    for (int e = 0; e < 6; ++e) t -= (double)Q.W[6 * k + e] * a[e];
    x[k] = t * (double)Q.di[k];
  }
#pragma unroll
  for (int k = K - 1; k >= 0; --k)
#pragma unroll
    for (int i = k + 1; i < K; ++i) x[k] -= (double)Q.L[mi_lx(i, k)] * x[i];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int i = 0; i < 6; ++i) a[i] += (double)Q.S[6 * k + i] * x[k];
}

__global__ __launch_bounds__(256) void k_mass_inverse(int nsets, int nb, const float *__restrict__ tab, const float *__restrict__ rows,
                                                      float *__restrict__ out) {
  __shared__ float slot[256 * MI_S], down[256 * GF_S];  // what a body hands up: Ia (21), pa (6) / its acceleration (6)
  __shared__ int s_anc[2][256], s_dep[2][256], s_max[4];
  const SetLane L = set_lane(nsets, nb);
  float *o = out + ((size_t)L.set * nb + L.body) * 6;  // (formed, not touched, by an inactive lane)
  if ((int)tab[0] != nb) {  // not this call's table (the same for every lane of the launch: no barrier is skipped by some)
    if (L.active)
      for (int k = 0; k < 6; ++k) o[k] = 0.0f;
    return;
  }
  const bool generalized = tab[3] != 0.0f;
  const GfTree T = gf_tree(tab, nb, L, s_anc, s_dep, s_max);
  MiJoint Q;
  double IA[21], pA[6];
  float r[6];
  int type = PD_JOINT_FIXED;
#pragma unroll
  for (int e = 0; e < 21; ++e) IA[e] = 0.0;
#pragma unroll
  for (int e = 0; e < 6; ++e) { pA[e] = 0.0; r[e] = 0.0f; }
  if (L.active) {
    const float *set_rows = rows + (size_t)L.set * nb * MI_ROW, *row = set_rows + (size_t)L.body * MI_ROW;
    const v3 o0 = ld3(set_rows);
    BodyState s;
    s.p = ld3(row); s.r = ld4(row + 3); s.w = V3(0, 0, 0); s.v = s.w;
    const JcJoint J = jc_joint<MI_ROW>(tab, nb, (int)tab[1], (int)tab[2], L.body, s, set_rows);
    type = J.type;
    const v3 d = (s.p - o0) + qrot(s.r, J.com);
    const v3 ra = type == PD_JOINT_FREE ? d : J.parent >= 0 ? (J.pp - o0) + qrot(J.qp, J.p_pj) : J.p_pj - o0;
    // the body's own spatial inertia in double from the fp32 row (rotm's polynomial, as qrot's): the shift to o0 adds m |d|^2 to an
    // inertia that may be 1e-4 of it
    const double m = (double)row[7], qx = s.r.x, qy = s.r.y, qz = s.r.z, qw = s.r.w, sq = 2.0 * qw * qw - 1.0;
    const double R[9] = {sq + 2.0 * qx * qx, 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
                         2.0 * (qx * qy + qw * qz), sq + 2.0 * qy * qy, 2.0 * (qy * qz - qw * qx),
                         2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), sq + 2.0 * qz * qz};
    double Is[9], RI[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Is[3 * i + j] = 0.5 * ((double)row[8 + 3 * i + j] + (double)row[8 + 3 * j + i]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) RI[3 * i + j] = R[3 * i] * Is[j] + R[3 * i + 1] * Is[3 + j] + R[3 * i + 2] * Is[6 + j];
    const double dv[3] = {d.x, d.y, d.z}, d2 = dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i; j < 3; ++j)
        IA[mi_ix(i, j)] = (RI[3 * i] * R[3 * j] + RI[3 * i + 1] * R[3 * j + 1] + RI[3 * i + 2] * R[3 * j + 2]) +
                          m * ((i == j ? d2 : 0.0) - dv[i] * dv[j]);
    IA[mi_ix(0, 4)] = -m * dv[2]; IA[mi_ix(0, 5)] = m * dv[1];  // m [d]x
    IA[mi_ix(1, 3)] = m * dv[2]; IA[mi_ix(1, 5)] = -m * dv[0];
    IA[mi_ix(2, 3)] = -m * dv[1]; IA[mi_ix(2, 4)] = m * dv[0];
    IA[mi_ix(3, 3)] = m; IA[mi_ix(4, 4)] = m; IA[mi_ix(5, 5)] = m;
#pragma unroll
    for (int k = 0; k < 6; ++k) r[k] = row[17 + k];
    if (type == PD_JOINT_FREE) {
      const v3 e0 = qrot(J.q_wj, V3(1, 0, 0)), e1 = qrot(J.q_wj, V3(0, 1, 0)), e2 = qrot(J.q_wj, V3(0, 0, 1)), zero = V3(0, 0, 0);
      mi_col(Q.S, e0, -cross(e0, ra)); mi_col(Q.S + 6, e1, -cross(e1, ra)); mi_col(Q.S + 12, e2, -cross(e2, ra));
      mi_col(Q.S + 18, zero, e0); mi_col(Q.S + 24, zero, e1); mi_col(Q.S + 30, zero, e2);
    } else if (type == PD_JOINT_REVOLUTE) {
      const v3 ah = qrot(J.q_wj, J.axis);
      mi_col(Q.S, ah, -cross(ah, ra));
    } else if (type == PD_JOINT_COMPOUND) {
      JcCompound C;
      jc_compound(J, false, C);
      v3 c0 = V3(1, 0, 0), c2 = C.a2;
      if (!generalized) {  // the columns of A G^-1
        const float id = 1.0f / (1.0f - C.s * C.s);
        c0 = (V3(1, 0, 0) - C.a2 * C.s) * id; c2 = (C.a2 - V3(C.s, 0, 0)) * id;
      }
      const v3 h0 = qrot(C.q_w, c0), h1 = qrot(C.q_w, C.a1), h2 = qrot(C.q_w, c2);
      mi_col(Q.S, h0, -cross(h0, ra)); mi_col(Q.S + 6, h1, -cross(h1, ra)); mi_col(Q.S + 12, h2, -cross(h2, ra));
    }
  }
  float *mine = slot + threadIdx.x * MI_S, *dn = down + threadIdx.x * GF_S;
#pragma unroll
  for (int e = 0; e < MI_S; ++e) mine[e] = 0.0f;  // (a malformed table may name a child that publishes later: it reads zeros)
#pragma unroll
  for (int e = 0; e < 6; ++e) dn[e] = 0.0f;
  for (int lev = T.maxd; lev >= 0; --lev) {
    __syncthreads();
    if (L.active && T.dep == lev) {
      for (int k = 0; k < T.nch; ++k) {
        const int c = (int)T.ch[k];
        if (c >= 0 && c < nb) {
          const float *cs = slot + (L.set_l * nb + c) * MI_S;
#pragma unroll
          for (int e = 0; e < 21; ++e) IA[e] += (double)cs[e];
#pragma unroll
          for (int e = 0; e < 6; ++e) pA[e] += (double)cs[21 + e];
        }
      }
      if (type == PD_JOINT_FREE) mi_factor<6>(IA, pA, r, Q);
      else if (type == PD_JOINT_COMPOUND) mi_factor<3>(IA, pA, r, Q);
      else if (type == PD_JOINT_REVOLUTE) mi_factor<1>(IA, pA, r, Q);
#pragma unroll
      for (int e = 0; e < 21; ++e) mine[e] = (float)IA[e];
#pragma unroll
      for (int e = 0; e < 6; ++e) mine[21 + e] = (float)pA[e];
    }
  }
  double a[6], x[6];
#pragma unroll
  for (int e = 0; e < 6; ++e) { a[e] = 0.0; x[e] = 0.0; }
  for (int lev = 0; lev <= T.maxd; ++lev) {
    __syncthreads();
    if (L.active && T.dep == lev) {
      if (T.parent >= 0) {
        const float *pp = down + (L.set_l * nb + T.parent) * GF_S;
#pragma unroll
        for (int e = 0; e < 6; ++e) a[e] = (double)pp[e];
      }
      if (type == PD_JOINT_FREE) mi_solve<6>(Q, a, x);
      else if (type == PD_JOINT_COMPOUND) mi_solve<3>(Q, a, x);
      else if (type == PD_JOINT_REVOLUTE) mi_solve<1>(Q, a, x);
#pragma unroll
      for (int e = 0; e < 6; ++e) dn[e] = (float)a[e];
    }
  }
  if (!L.active) return;
#pragma unroll
  for (int k = 0; k < 6; ++k) o[k] = (float)x[k];
}

// ---- PD_POSE_MASS_MATRIX: the joint-space mass matrix H = sum_b J_b^T diag(R_b sym(I_b) R_b^T, m_b) J_b of a state (J =
// PD_POSE_BODY_TWIST's Jacobian in the table's mode: the matrix whose inverse PD_POSE_MASS_INVERSE applies) by the composite-rigid-body
// recursion, from rows (p, q xyzw, m, I row-major) -> [n / nb][nqd * nqd] row-major in the joint_qd layout, and its vector-Jacobian
// product with respect to the rows.  The frame, the spatial inertia (mi_ix) and the motion subspace S_i are k_mass_inverse's: world axes
// about o0, spatial vectors (angular, linear at o0).  (That kernel keeps its own lines: sharing them changes its instruction stream.)
//   up, deepest level first   Ic_i = I_i + sum_children Ic_c   (the table's child order; 21 doubles handed up per body)
//   per body i with dofs      F_i = Ic_i S_i                   (6 x K_i)
//   walk j = i, pi(i), ...    H[dofs_j, dofs_i] = S_j^T F_i and its transpose, both from one computed value
// Every lane publishes its S (fp32, at most 36 floats) in LDS for its descendants' walks.  The set's lanes zero its nqd^2 floats in a
// fixed order first; the barriers of the up sweep separate that from the walks' writes, after which every float between related dofs
// has one writing lane and every other one stays exactly 0.  A walk is bounded by nb steps (a malformed table may hold a cycle) and a
// joint's dofs lie inside [0, nqd) or it is FIXED (jc_joint): nothing is indexed outside the set.  A table of another nb: zeros.
// Precision: rows, frames and S are fp32; the body's inertia, the sums over children, F and the products are double and the composite
// is handed over in double (rounding it to fp32 at each hand-over costs 1e-5 of sqrt(H_aa H_bb) on a long chain: DESIGN.md section 8).
// VJP of <G, H>, G arbitrary, Gs = (G + G^T) / 2:
//   A_i = sum_{j in anc*(i)} S_j Gs_ji;   Q_i = A_i S_i^T + S_i A_i^T - S_i Gs_ii S_i^T;   dL/dI_b = P_b = sum_{i in anc*(b)} Q_i
//   dL/dS_i = Z_i = 2 (Ic_i A_i + sum_{k in desc(i)} F_k Gs_ki)
// a column of S_i at a time: the ancestor walk, the gather over the set's bodies k (in body order; k is a descendant when walking up
// depth(k) - depth(i) parents from k ends at i), and the column's share of Q_i and of the adjoints of the joint's axes and anchor.
// Then P_b by an ancestor sum from the roots down (21 doubles), P_b into (p, q, m, sym I) of the body, Z into the frames S_i depends
// on -- the body's own pose, the parent's, jc_compound's axes as k_body_twist_vjp differentiates them --, the parent-side pose adjoint
// handed over as k_joint_coords_vjp does.  o0 is a constant of the adjoint: H does not depend on the reference point.  No atomics.
enum { MM_ROW = 17, MM_S = 37 };  // floats of a row / of an LDS slot of S or F (36 used; odd stride)
struct MmBody { BodyState s; JcJoint J; JcCompound C; v3 d, ra, c0, c2; int K; };  // c0, c2: the COMPOUND columns 0 and 2 in the offset frame
// The body's pose, joint frames and motion subspace (S: 36 floats, zero past the joint's columns)
__device__ __forceinline__ void mm_load(const float *tab, int nb, int body, const float *set_rows, bool generalized, MmBody &B, float *S) {
  const float *row = set_rows + (size_t)body * MM_ROW;
  const v3 o0 = ld3(set_rows);
  B.s.p = ld3(row); B.s.r = ld4(row + 3); B.s.w = V3(0, 0, 0); B.s.v = B.s.w;
  B.J = jc_joint<MM_ROW>(tab, nb, (int)tab[1], (int)tab[2], body, B.s, set_rows);
  const JcJoint &J = B.J;
  B.d = (B.s.p - o0) + qrot(B.s.r, J.com);
  B.ra = J.type == PD_JOINT_FREE ? B.d : J.parent >= 0 ? (J.pp - o0) + qrot(J.qp, J.p_pj) : J.p_pj - o0;
  B.c0 = V3(1, 0, 0); B.c2 = V3(0, 0, 1); B.K = 0;
  v3 u0 = V3(0, 0, 0), u1 = u0, u2 = u0;  // the joint's axes in world axes
  if (J.type == PD_JOINT_FREE) {
    u0 = qrot(J.q_wj, V3(1, 0, 0)); u1 = qrot(J.q_wj, V3(0, 1, 0)); u2 = qrot(J.q_wj, V3(0, 0, 1));
    B.K = 6;
  } else if (J.type == PD_JOINT_REVOLUTE) {
    u0 = qrot(J.q_wj, J.axis);
    B.K = 1;
  } else if (J.type == PD_JOINT_COMPOUND) {
    jc_compound(J, false, B.C);
    B.c2 = B.C.a2;
    if (!generalized) {  // the columns of A G^-1
      const float id = 1.0f / (1.0f - B.C.s * B.C.s);
      B.c0 = (V3(1, 0, 0) - B.C.a2 * B.C.s) * id; B.c2 = (B.C.a2 - V3(B.C.s, 0, 0)) * id;
    }
    u0 = qrot(B.C.q_w, B.c0); u1 = qrot(B.C.q_w, B.C.a1); u2 = qrot(B.C.q_w, B.c2);
    B.K = 3;
  }
  // (every store unconditional, at a constant index: an axis the joint does not have is zero)
  const v3 zero = V3(0, 0, 0);
  const bool free = B.K == 6;
  mi_col(S, u0, -cross(u0, B.ra)); mi_col(S + 6, u1, -cross(u1, B.ra)); mi_col(S + 12, u2, -cross(u2, B.ra));
  mi_col(S + 18, zero, free ? u0 : zero); mi_col(S + 24, zero, free ? u1 : zero); mi_col(S + 30, zero, free ? u2 : zero);
}
__device__ __forceinline__ void mm_rotm(qt q, double *R) {  // rotm's polynomial, as qrot's, in double
  const double qx = q.x, qy = q.y, qz = q.z, qw = q.w, sq = 2.0 * qw * qw - 1.0;
  R[0] = sq + 2.0 * qx * qx; R[1] = 2.0 * (qx * qy - qw * qz); R[2] = 2.0 * (qx * qz + qw * qy);
  R[3] = 2.0 * (qx * qy + qw * qz); R[4] = sq + 2.0 * qy * qy; R[5] = 2.0 * (qy * qz - qw * qx);
  R[6] = 2.0 * (qx * qz - qw * qy); R[7] = 2.0 * (qy * qz + qw * qx); R[8] = sq + 2.0 * qz * qz;
}
__device__ __forceinline__ void mm_sym(const float *row, double *Is) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Is[3 * i + j] = 0.5 * ((double)row[8 + 3 * i + j] + (double)row[8 + 3 * j + i]);
}
// The body's own spatial inertia about o0 in double from the fp32 row (the shift adds m |d|^2 to an inertia that may be 1e-4 of it)
__device__ __forceinline__ void mm_inertia(const float *row, qt q, v3 d, double *IA) {
  const double m = (double)row[7];
  double R[9], Is[9], RI[9];
  mm_rotm(q, R);
  mm_sym(row, Is);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) RI[3 * i + j] = R[3 * i] * Is[j] + R[3 * i + 1] * Is[3 + j] + R[3 * i + 2] * Is[6 + j];
  const double dv[3] = {d.x, d.y, d.z}, d2 = dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j)
      IA[mi_ix(i, j)] = (RI[3 * i] * R[3 * j] + RI[3 * i + 1] * R[3 * j + 1] + RI[3 * i + 2] * R[3 * j + 2]) +
                        m * ((i == j ? d2 : 0.0) - dv[i] * dv[j]);
  IA[mi_ix(0, 3)] = 0.0; IA[mi_ix(1, 4)] = 0.0; IA[mi_ix(2, 5)] = 0.0;
  IA[mi_ix(0, 4)] = -m * dv[2]; IA[mi_ix(0, 5)] = m * dv[1];  // m [d]x
  IA[mi_ix(1, 3)] = m * dv[2]; IA[mi_ix(1, 5)] = -m * dv[0];
  IA[mi_ix(2, 3)] = -m * dv[1]; IA[mi_ix(2, 4)] = m * dv[0];
  IA[mi_ix(3, 3)] = m; IA[mi_ix(4, 4)] = m; IA[mi_ix(5, 5)] = m;
  IA[mi_ix(3, 4)] = 0.0; IA[mi_ix(3, 5)] = 0.0; IA[mi_ix(4, 5)] = 0.0;
}
// Composite inertias: levels deepest first, a body adds its children's 21 doubles in the table's child order and publishes its own.
__device__ __forceinline__ void mm_up(double *comp, const GfTree &T, const SetLane &L, int nb, double *IA) {
  double *cm = comp + threadIdx.x * 21;
#pragma unroll
  for (int e = 0; e < 21; ++e) cm[e] = 0.0;  // (a malformed table may name a child that publishes later: it reads zeros)
  for (int lev = T.maxd; lev >= 0; --lev) {
    __syncthreads();
    if (L.active && T.dep == lev) {
      for (int k = 0; k < T.nch; ++k) {
        const int c = (int)T.ch[k];
        if (c >= 0 && c < nb) {
          const double *cs = comp + (L.set_l * nb + c) * 21;
#pragma unroll
          for (int e = 0; e < 21; ++e) IA[e] += cs[e];
        }
      }
#pragma unroll
      for (int e = 0; e < 21; ++e) cm[e] = IA[e];
    }
  }
}
template <int K>
__device__ __forceinline__ void mm_force(const double *IA, const float *S, double *F) {  // F = Ic S, column k at [6 k ..]
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double t = IA[mi_ix(i, 0)] * (double)S[6 * k];
#pragma unroll
      for (int j = 1; j < 6; ++j) t += IA[mi_ix(i, j)] * (double)S[6 * k + j];
      F[6 * k + i] = t;
    }
}
// The blocks of H the body's dofs share with its own and its ancestors' (base: the set's first lane).  Every index is a constant.
template <int K>
__device__ __forceinline__ void mm_walk(const double *IA, const float *S, const float *Ssh, const int *s_par, const int *s_k, const int *s_qd,
                                        int base, int body, int qds, int nb, int nqd, float *o) {
  double F[6 * K];
  mm_force<K>(IA, S, F);
#pragma unroll
  for (int a = 0; a < K; ++a)
#pragma unroll
    for (int b = a; b < K; ++b) {
      double h = 0.0;
#pragma unroll
      for (int e = 0; e < 6; ++e) h += (double)S[6 * a + e] * F[6 * b + e];
      o[(size_t)(qds + a) * nqd + (qds + b)] = (float)h;
      o[(size_t)(qds + b) * nqd + (qds + a)] = (float)h;
    }
  int j = s_par[base + body];
  for (int step = 1; j >= 0 && step < nb; ++step) {
    const int Kj = s_k[base + j], dj = s_qd[base + j];
    const float *Sj = Ssh + (base + j) * MM_S;
#pragma unroll
    for (int a = 0; a < 6; ++a)
      if (a < Kj) {
        double sj[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) sj[e] = (double)Sj[6 * a + e];
#pragma unroll
        for (int b = 0; b < K; ++b) {
          double h = 0.0;
#pragma unroll
          for (int e = 0; e < 6; ++e) h += sj[e] * F[6 * b + e];
          o[(size_t)(dj + a) * nqd + (qds + b)] = (float)h;
          o[(size_t)(qds + b) * nqd + (dj + a)] = (float)h;
        }
      }
    j = s_par[base + j];
  }
}

__global__ __launch_bounds__(256) void k_mass_matrix(int nsets, int nb, const float *__restrict__ tab, const float *__restrict__ rows,
                                                     float *__restrict__ out) {
  __shared__ float Ssh[256 * MM_S];  // lane -> its motion subspace
  __shared__ double comp[256 * 21];  // lane -> its composite inertia
  __shared__ int s_anc[2][256], s_dep[2][256], s_max[4];
  const SetLane L = set_lane(nsets, nb);
  const int nqd = max((int)tab[2], 0);
  const size_t nn = (size_t)nqd * nqd;
  float *o = out + (size_t)L.set * nn;  // (formed, not touched, by an inactive lane)
  if (L.active)
    for (size_t k = (size_t)L.body; k < nn; k += (size_t)nb) o[k] = 0.0f;
  if ((int)tab[0] != nb) return;  // not this call's table (the same for every lane of the launch: no barrier is skipped by some)
  const bool generalized = tab[3] != 0.0f;
  const GfTree T = gf_tree(tab, nb, L, s_anc, s_dep, s_max);
  MmBody B;
  float S[36];
  double IA[21];
#pragma unroll
  for (int e = 0; e < 36; ++e) S[e] = 0.0f;
#pragma unroll
  for (int e = 0; e < 21; ++e) IA[e] = 0.0;
  B.K = 0; B.J.qds = 0;
  if (L.active) {
    const float *set_rows = rows + (size_t)L.set * nb * MM_ROW;
    mm_load(tab, nb, L.body, set_rows, generalized, B, S);
    mm_inertia(set_rows + (size_t)L.body * MM_ROW, B.s.r, B.d, IA);
  }
  int *s_par = s_anc[0], *s_k = s_anc[1], *s_qd = s_dep[0];  // (gf_tree is done with them: its last barrier is behind every read)
  s_par[threadIdx.x] = T.parent; s_k[threadIdx.x] = B.K; s_qd[threadIdx.x] = B.J.qds;
  float *mine = Ssh + threadIdx.x * MM_S;
#pragma unroll
  for (int e = 0; e < 36; ++e) mine[e] = S[e];
  mm_up(comp, T, L, nb, IA);  // (its barriers also stand between the zeros above and the walks' writes, and publish S)
  if (!L.active) return;
  const int base = L.set_l * nb;
  if (B.K == 6) mm_walk<6>(IA, S, Ssh, s_par, s_k, s_qd, base, L.body, B.J.qds, nb, nqd, o);
  else if (B.K == 3) mm_walk<3>(IA, S, Ssh, s_par, s_k, s_qd, base, L.body, B.J.qds, nb, nqd, o);
  else if (B.K == 1) mm_walk<1>(IA, S, Ssh, s_par, s_k, s_qd, base, L.body, B.J.qds, nb, nqd, o);
}

// g_b [n][17]: the raw partials of <g_out, out> with respect to (p, q, m, I) of every body; the inertia's are those of sym(I).
__global__ __launch_bounds__(256) void k_mass_matrix_vjp(int nsets, int nb, const float *__restrict__ tab, const float *__restrict__ rows,
                                                         const float *__restrict__ g_out, float *__restrict__ g_b) {
  __shared__ float Ssh[256 * MM_S], Fsh[256 * MM_S], pslot[256 * GF_S];  // S / F = Ic S / the parent-side pose adjoint
  __shared__ double comp[256 * 21];                                       // composite inertias up, then the ancestor sums of Q down
  __shared__ int s_anc[2][256], s_dep[2][256], s_max[4];
  const SetLane L = set_lane(nsets, nb);
  float *dst = g_b + ((size_t)L.set * nb + L.body) * MM_ROW;  // (formed, not touched, by an inactive lane)
  if ((int)tab[0] != nb) {
    if (L.active)
      for (int k = 0; k < MM_ROW; ++k) dst[k] = 0.0f;
    return;
  }
  const int nqd = max((int)tab[2], 0);
  const bool generalized = tab[3] != 0.0f;
  const GfTree T = gf_tree(tab, nb, L, s_anc, s_dep, s_max);
  MmBody B;
  float S[36];
  double IA[21];
#pragma unroll
  for (int e = 0; e < 36; ++e) S[e] = 0.0f;
#pragma unroll
  for (int e = 0; e < 21; ++e) IA[e] = 0.0;
  B.K = 0; B.J.qds = 0;
  const float *row = rows;
  if (L.active) {
    const float *set_rows = rows + (size_t)L.set * nb * MM_ROW;
    row = set_rows + (size_t)L.body * MM_ROW;
    mm_load(tab, nb, L.body, set_rows, generalized, B, S);
    mm_inertia(row, B.s.r, B.d, IA);
  }
  int *s_par = s_anc[0], *s_k = s_anc[1], *s_qd = s_dep[0], *s_dp = s_dep[1];  // (gf_tree is done with them)
  s_par[threadIdx.x] = T.parent; s_k[threadIdx.x] = B.K; s_qd[threadIdx.x] = B.J.qds; s_dp[threadIdx.x] = T.dep;
  float *mine = Ssh + threadIdx.x * MM_S, *fmine = Fsh + threadIdx.x * MM_S;
#pragma unroll
  for (int e = 0; e < 36; ++e) mine[e] = S[e];
  mm_up(comp, T, L, nb, IA);
  {
    double F[36];
#pragma unroll
    for (int e = 0; e < 36; ++e) F[e] = 0.0;
    if (B.K == 6) mm_force<6>(IA, S, F);
    else if (B.K == 3) mm_force<3>(IA, S, F);
    else if (B.K == 1) mm_force<1>(IA, S, F);
#pragma unroll
    for (int e = 0; e < 36; ++e) fmine[e] = (float)F[e];
  }
  __syncthreads();  // F is published; nobody reads a composite any more
  const int base = L.set_l * nb, K = B.K, qds = B.J.qds;
  double Q[21];
#pragma unroll
  for (int e = 0; e < 21; ++e) Q[e] = 0.0;
  v3 gu0 = V3(0, 0, 0), gu1 = gu0, gu2 = gu0, adj_ra = gu0;  // the adjoints of the joint's three axes and of its anchor
  if (L.active) {
    const float *G = g_out + (size_t)L.set * nqd * nqd;
    for (int b = 0; b < K; ++b) {
      const size_t cb = (size_t)(qds + b);
      const float *sb = mine + 6 * b;
      double a[6], self[6], z[6];
#pragma unroll
      for (int e = 0; e < 6; ++e) self[e] = 0.0;
      for (int c = 0; c < K; ++c) {
        const size_t cc = (size_t)(qds + c);
        const double gs = 0.5 * ((double)G[cc * nqd + cb] + (double)G[cb * nqd + cc]);
#pragma unroll
        for (int e = 0; e < 6; ++e) self[e] += (double)mine[6 * c + e] * gs;
      }
#pragma unroll
      for (int e = 0; e < 6; ++e) a[e] = self[e];
      int j = T.parent;
      for (int step = 1; j >= 0 && step < nb; ++step) {
        const int Kj = s_k[base + j], dj = s_qd[base + j];
        const float *Sj = Ssh + (base + j) * MM_S;
        for (int c = 0; c < Kj; ++c) {
          const size_t cc = (size_t)(dj + c);
          const double gs = 0.5 * ((double)G[cc * nqd + cb] + (double)G[cb * nqd + cc]);
#pragma unroll
          for (int e = 0; e < 6; ++e) a[e] += (double)Sj[6 * c + e] * gs;
        }
        j = s_par[base + j];
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) {  // Q += a' s^T + s a'^T, a' = a - self / 2 (the own block counts once)
        const double ai = a[i] - 0.5 * self[i], si = (double)sb[i];
#pragma unroll
        for (int jj = i; jj < 6; ++jj) Q[mi_ix(i, jj)] += ai * (double)sb[jj] + si * (a[jj] - 0.5 * self[jj]);
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double t = IA[mi_ix(i, 0)] * a[0];
#pragma unroll
        for (int jj = 1; jj < 6; ++jj) t += IA[mi_ix(i, jj)] * a[jj];
        z[i] = t;
      }
      for (int k = 0; k < nb; ++k) {  // the descendants, in body order
        const int Kk = s_k[base + k], up = s_dp[base + k] - T.dep;
        if (Kk == 0 || up <= 0) continue;
        int anc = k;
        for (int s = 0; s < up && anc >= 0; ++s) anc = s_par[base + anc];
        if (anc != L.body) continue;
        const int dk = s_qd[base + k];
        const float *Fk = Fsh + (base + k) * MM_S;
        for (int c = 0; c < Kk; ++c) {
          const size_t cc = (size_t)(dk + c);
          const double gs = 0.5 * ((double)G[cc * nqd + cb] + (double)G[cb * nqd + cc]);
#pragma unroll
          for (int e = 0; e < 6; ++e) z[e] += (double)Fk[6 * c + e] * gs;
        }
      }
      const v3 za = V3((float)(2.0 * z[0]), (float)(2.0 * z[1]), (float)(2.0 * z[2]));
      const v3 zl = V3((float)(2.0 * z[3]), (float)(2.0 * z[4]), (float)(2.0 * z[5]));
      const bool lin = K == 6 && b >= 3;  // a FREE joint's column (0, e_k)
      v3 g = zl;
      if (!lin) {  // the column (u, ra x u)
        g = za;
        adj_cross(B.ra, V3(sb[0], sb[1], sb[2]), adj_ra, g, zl);
      }
      const int kk = lin ? b - 3 : b;
      if (kk == 0) gu0 += g;
      else if (kk == 1) gu1 += g;
      else gu2 += g;
    }
  }
  // P_b = the sum of Q over the body and its ancestors: levels from the roots down
  double *cm = comp + threadIdx.x * 21;
#pragma unroll
  for (int e = 0; e < 21; ++e) cm[e] = Q[e];
  for (int lev = 1; lev <= T.maxd; ++lev) {
    __syncthreads();
    if (L.in_set && T.dep == lev && T.parent >= 0) {
      const double *pp = comp + (base + T.parent) * 21;
#pragma unroll
      for (int e = 0; e < 21; ++e) { Q[e] += pp[e]; cm[e] = Q[e]; }
    }
  }
  v3 own_p = V3(0, 0, 0), par_p = own_p;
  qt own_q = Q4(0, 0, 0, 0), par_q = own_q;
  float g_m = 0.0f, g_I[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) g_I[e] = 0.0f;
  if (L.active) {
    const JcJoint &J = B.J;
    // the body's own spatial inertia [[R Is R^T + m (|d|^2 1 - d d^T), m [d]x], [-m [d]x, m 1]] against P (a full symmetric matrix)
    const double m = (double)row[7], dv[3] = {B.d.x, B.d.y, B.d.z}, d2 = dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2];
    double R[9], Is[9], PR[9], RI[9];
    mm_rotm(B.s.r, R);
    mm_sym(row, Is);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        PR[3 * i + j] = Q[mi_ix(i, 0)] * R[j] + Q[mi_ix(i, 1)] * R[3 + j] + Q[mi_ix(i, 2)] * R[6 + j];
        RI[3 * i + j] = R[3 * i] * Is[j] + R[3 * i + 1] * Is[3 + j] + R[3 * i + 2] * Is[6 + j];
      }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) g_I[3 * i + j] = (float)(R[i] * PR[j] + R[3 + i] * PR[3 + j] + R[6 + i] * PR[6 + j]);  // R^T P_aa R
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // adj R = 2 P_aa R Is; column k of R is qrot(q, e_k)
      v3 gk;
      gk.x = (float)(2.0 * (Q[mi_ix(0, 0)] * RI[k] + Q[mi_ix(0, 1)] * RI[3 + k] + Q[mi_ix(0, 2)] * RI[6 + k]));
      gk.y = (float)(2.0 * (Q[mi_ix(1, 0)] * RI[k] + Q[mi_ix(1, 1)] * RI[3 + k] + Q[mi_ix(1, 2)] * RI[6 + k]));
      gk.z = (float)(2.0 * (Q[mi_ix(2, 0)] * RI[k] + Q[mi_ix(2, 1)] * RI[3 + k] + Q[mi_ix(2, 2)] * RI[6 + k]));
      adj_qrot_q(B.s.r, V3(k == 0 ? 1.f : 0.f, k == 1 ? 1.f : 0.f, k == 2 ? 1.f : 0.f), own_q, gk);
    }
    const double tr = Q[mi_ix(0, 0)] + Q[mi_ix(1, 1)] + Q[mi_ix(2, 2)];
    double Pd[3], dPd = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      Pd[i] = Q[mi_ix(i, 0)] * dv[0] + Q[mi_ix(i, 1)] * dv[1] + Q[mi_ix(i, 2)] * dv[2];
      dPd += dv[i] * Pd[i];
    }
    const double vx[3] = {Q[mi_ix(2, 4)] - Q[mi_ix(1, 5)], Q[mi_ix(0, 5)] - Q[mi_ix(2, 3)], Q[mi_ix(1, 3)] - Q[mi_ix(0, 4)]};  // the m [d]x blocks
    g_m = (float)(tr * d2 - dPd + 2.0 * (dv[0] * vx[0] + dv[1] * vx[1] + dv[2] * vx[2]) + Q[mi_ix(3, 3)] + Q[mi_ix(4, 4)] + Q[mi_ix(5, 5)]);
    v3 adj_d = V3((float)(2.0 * m * (tr * dv[0] - Pd[0] + vx[0])), (float)(2.0 * m * (tr * dv[1] - Pd[1] + vx[1])),
                  (float)(2.0 * m * (tr * dv[2] - Pd[2] + vx[2])));
    // the joint's axes and anchor
    qt adj_q_wj = Q4(0, 0, 0, 0);
    if (J.type == PD_JOINT_FREE) {
      adj_qrot_q(J.q_wj, V3(1, 0, 0), adj_q_wj, gu0);
      adj_qrot_q(J.q_wj, V3(0, 1, 0), adj_q_wj, gu1);
      adj_qrot_q(J.q_wj, V3(0, 0, 1), adj_q_wj, gu2);
      adj_d += adj_ra;  // (a FREE joint's anchor is d)
    } else if (J.type == PD_JOINT_REVOLUTE) {
      adj_qrot_q(J.q_wj, J.axis, adj_q_wj, gu0);
    } else if (J.type == PD_JOINT_COMPOUND) {
      const JcCompound &C = B.C;
      qt adj_q_w = Q4(0, 0, 0, 0), adj_r_err = adj_q_w;
      v3 adj_c0 = V3(0, 0, 0), adj_a1 = adj_c0, adj_c2 = adj_c0;
      adj_qrot(C.q_w, B.c0, adj_q_w, adj_c0, gu0);
      adj_qrot(C.q_w, C.a1, adj_q_w, adj_a1, gu1);
      adj_qrot(C.q_w, B.c2, adj_q_w, adj_c2, gu2);
      v3 adj_a2 = adj_c2;
      if (!generalized) {  // c_0 = (e_0 - s a_2) id, c_2 = (a_2 - s e_0) id, s = a_2.x, id = 1 / (1 - s^2)
        const float id = 1.0f / (1.0f - C.s * C.s);
        adj_a2 = (adj_c2 - adj_c0 * C.s) * id;
        adj_a2.x += -id * (dot(C.a2, adj_c0) + adj_c2.x) + (dot(B.c0, adj_c0) + dot(B.c2, adj_c2)) * (2.0f * C.s * id);
      }
      adj_qmul_a(J.q_off, adj_q_wj, adj_q_w);
      // the axis chain and the decomposition, as k_body_twist_vjp
      float adj_ang[3] = {0.f, 0.f, 0.f};
      qt adj_q10 = Q4(0, 0, 0, 0), adj_q_1 = adj_q10, adj_q_0 = adj_q10;
      adj_qrot_q(C.q10, V3(0, 0, 1), adj_q10, adj_a2);
      adj_qmul(C.q_1, C.q_0, adj_q_1, adj_q_0, adj_q10);
      adj_q_axis_angle(C.a1, C.ang[1], adj_a1, adj_ang[1], adj_q_1);
      adj_qrot_q(C.q_0, V3(0, 1, 0), adj_q_0, adj_a1);
      adj_q_axis_angle_ang(V3(1, 0, 0), C.ang[0], adj_ang[0], adj_q_0);
      qt adj_q_pc = Q4(0, 0, 0, 0), adj_qa = adj_q_pc;
      quat_decompose_adj(C.q_pc, C.c0, C.c1, C.c2, adj_ang, adj_q_pc);
      adj_qmul_a(J.q_off, adj_qa, adj_q_pc);
      adj_qmul_b(qconj(J.q_off), adj_r_err, adj_qa);
      qt adj_cq = Q4(0, 0, 0, 0);
      adj_qmul(qconj(J.q_wj), B.s.r, adj_cq, own_q, adj_r_err);  // r_err = conj(q_wj) q_c
      adj_q_wj += qconj(adj_cq);
    }
    if (J.type != PD_JOINT_FREE && J.parent >= 0) {  // ra = (p_p - o0) + R(q_p) p_pj
      par_p += adj_ra;
      adj_qrot_q(J.qp, J.p_pj, par_q, adj_ra);
    }
    if (J.parent >= 0) adj_qmul_a(J.q_pj, par_q, adj_q_wj);  // q_wj = q_p q_pj
    own_p += adj_d;  // d = (p_b - o0) + R(q_b) com_b
    adj_qrot_q(B.s.r, J.com, own_q, adj_d);
  }
  float *ps = pslot + threadIdx.x * GF_S;
  ps[0] = par_p.x; ps[1] = par_p.y; ps[2] = par_p.z; ps[3] = par_q.x; ps[4] = par_q.y; ps[5] = par_q.z; ps[6] = par_q.w;
  __syncthreads();
  if (!L.active) return;
  for (int k = 0; k < T.nch; ++k) {
    const int c = (int)T.ch[k];
    if (c >= 0 && c < nb) {
      const float *cs = pslot + (base + c) * GF_S;
      own_p += ld3(cs); own_q += ld4(cs + 3);
    }
  }
  dst[0] = own_p.x; dst[1] = own_p.y; dst[2] = own_p.z;
  dst[3] = own_q.x; dst[4] = own_q.y; dst[5] = own_q.z; dst[6] = own_q.w;
  dst[7] = g_m;
#pragma unroll
  for (int k = 0; k < 9; ++k) dst[8 + k] = g_I[k];
}

template <int OP>
int launch_pose(int n, const float *a, int a_bcast, const float *b, float *out, const float *g_out, float *g_a, float *g_b, hipStream_t st) {
  const dim3 grid((n + 255) / 256), block(256);
  constexpr bool project = OP == OP_PROJECT || OP == OP_PROJECT_POINT;
  const int a_sel = project ? a_bcast : (a_bcast ? 0 : Shape<OP>::NA);  // (a_offset)
  if (out)
    hipLaunchKernelGGL(k_pose_fwd<OP>, grid, block, 0, st, n, a, a_sel, b, out);
  else
    hipLaunchKernelGGL(k_pose_vjp<OP>, grid, block, 0, st, n, a, a_sel, b, g_out, g_a, g_b);
  if (hipGetLastError() == hipSuccess) return 0;
  pd_set_error("pd_pose_op: the kernel launch failed");
  return 2;
}

// The tabled ops: a = the op's table, a_bcast = nb (the group size g: element i is body i % g of state set i / g), b = rows [n][13]
// ([n][23] = (state, mass, inertia) for the centroidal op, [n][25] = (state, controls) for the joint wrench).  One launcher serves them; what differs per op is a row of TABLED:
//   ground wrench      out / g_out [n][6], g_a [n][nmat][4]; any nb
//   joint coordinates  out / g_out [n / nb][nq + nqd]; no g_a
//   centroidal         out / g_out [n / nb][16], g_b [n][23]; no g_a
//   contact state      out / g_out [n][8]; the ground wrench's contact table, no g_a; any nb
//   joint wrench       b / g_b [n][25] = (state, the joint's controls), out / g_out [n][6]; the joint-force table, no g_a
//   generalized force  b / g_b [n][13] = (pose, wrench), out / g_out [n / nb][nqd]; the joint table, no g_a
//   body twist         b / g_b [n][13] = (pose, the joint's rates in six slots), out / g_out [n][6]; the joint table, no g_a
//   body acceleration  b / g_b [n][19] = (state, the derivatives of the joint's rate slots), out / g_out [n][6]; the joint table, no g_a
//   mass inverse       b [n][23] = (pose, mass, inertia, the joint's force slots), out [n][6]; the joint table; forward only -- the
//                      gradient is composed by the caller from this op and the body twist, pd_pose_op_vjp refuses the code by name
//   mass matrix        b / g_b [n][17] = (pose, mass, inertia), out / g_out [n / nb][nqd * nqd]; the joint table, no g_a
enum Geometry { GEO_WAVE, GEO_LANE, GEO_SETS };  // a wavefront per element / a lane per element / 256 / nb whole state sets per workgroup
struct TabledOp { int op; const char *name, *table; int max_nb; bool has_g_a; Geometry fwd, vjp; const char *composed = nullptr; };  // max_nb 0: no cap (GEO_SETS needs one <= 256); composed: no VJP kernel, and from what the gradient is put together
constexpr TabledOp TABLED[] = {
    {PD_POSE_GROUND_WRENCH, "PD_POSE_GROUND_WRENCH", "contact", 0, true, GEO_WAVE, GEO_WAVE},
    {PD_POSE_JOINT_COORDS, "PD_POSE_JOINT_COORDS", "joint", JC_MAXNB, false, GEO_LANE, GEO_SETS},
    {PD_POSE_CENTROIDAL, "PD_POSE_CENTROIDAL", "mass", CT_MAXNB, false, GEO_SETS, GEO_SETS},
    {PD_POSE_CONTACT_STATE, "PD_POSE_CONTACT_STATE", "contact", 0, false, GEO_WAVE, GEO_WAVE},
    {PD_POSE_JOINT_WRENCH, "PD_POSE_JOINT_WRENCH", "jointforce", JC_MAXNB, false, GEO_SETS, GEO_SETS},
    {PD_POSE_GENERALIZED_FORCE, "PD_POSE_GENERALIZED_FORCE", "joint", JC_MAXNB, false, GEO_SETS, GEO_SETS},
    {PD_POSE_BODY_TWIST, "PD_POSE_BODY_TWIST", "joint", JC_MAXNB, false, GEO_SETS, GEO_SETS},
    {PD_POSE_BODY_ACCEL, "PD_POSE_BODY_ACCEL", "joint", JC_MAXNB, false, GEO_SETS, GEO_SETS},
    {PD_POSE_MASS_INVERSE, "PD_POSE_MASS_INVERSE", "joint", JC_MAXNB, false, GEO_SETS, GEO_SETS,
     "the gradient is composed from pd_pose_op(21) and PD_POSE_BODY_TWIST (17)"},
    {PD_POSE_MASS_MATRIX, "PD_POSE_MASS_MATRIX", "joint", JC_MAXNB, false, GEO_SETS, GEO_SETS},
};

template <class... A>
int refuse(const char *fmt, A... args) {  // pd_set_error of a formatted message
  char msg[160];
  snprintf(msg, sizeof msg, fmt, args...);
  return pd_set_error(msg);
}

int launch_tabled(const TabledOp &T, int n, const float *tab, int nb, const float *rows, float *out, const float *g_out, float *g_a,
                  float *g_b, hipStream_t st, bool vjp) {
  if (nb <= 0 || n % nb != 0)  // before the n == 0 return, like the projection ops: a bad group size is refused at every n
    return pd_set_error("pd_pose_op: n % g != 0 -- the element count must be a multiple of the bodies per state set, a_broadcast = nb >= 1");
  if (T.max_nb && nb > T.max_nb) return refuse("pd_pose_op: %s serves at most %d bodies per state set", T.name, T.max_nb);
  if (g_a && !T.has_g_a)  // before the n == 0 return, too
    return refuse("pd_pose_op_vjp: %s has no gradient for its %s table -- g_a_dev must be NULL", T.name, T.table);
  if (vjp && T.composed) return refuse("pd_pose_op_vjp: %s has no VJP kernel -- %s", T.name, T.composed);  // at every n, before any launch
  if (n == 0) return 0;
  if (!tab || !rows) return pd_set_error("pd_pose_op: a NULL operand");
  if ((size_t)tab & 15) return refuse("pd_pose_op: the %s table a_dev must be 16-byte aligned", T.table);
  // What the kernel counts (its first argument) and how many of them a workgroup of 256 lanes serves: elements, or whole state sets
  const Geometry geo = out ? T.fwd : T.vjp;
  const int count = geo == GEO_SETS ? n / nb : n;
  const int per_wg = geo == GEO_WAVE ? 4 : geo == GEO_LANE ? 256 : 256 / nb;
  const dim3 grid((unsigned)((count + per_wg - 1) / per_wg)), block(256);
  switch (T.op) {
    case PD_POSE_GROUND_WRENCH:
      if (out) hipLaunchKernelGGL(k_ground_wrench_fwd, grid, block, 0, st, count, nb, tab, rows, out);
      else hipLaunchKernelGGL(k_ground_wrench_vjp, grid, block, 0, st, count, nb, tab, rows, g_out, g_a, g_b);
      break;
    case PD_POSE_JOINT_COORDS:
      if (out) hipLaunchKernelGGL(k_joint_coords_fwd, grid, block, 0, st, count, nb, tab, rows, out);
      else hipLaunchKernelGGL(k_joint_coords_vjp, grid, block, 0, st, count, nb, tab, rows, g_out, g_b);
      break;
    case PD_POSE_CENTROIDAL:
      if (out) hipLaunchKernelGGL(k_centroidal_fwd, grid, block, 0, st, count, nb, tab, rows, out);
      else hipLaunchKernelGGL(k_centroidal_vjp, grid, block, 0, st, count, nb, tab, rows, g_out, g_b);
      break;
    case PD_POSE_JOINT_WRENCH:
      if (out) hipLaunchKernelGGL(k_joint_wrench_fwd, grid, block, 0, st, count, nb, tab, rows, out);
      else hipLaunchKernelGGL(k_joint_wrench_vjp, grid, block, 0, st, count, nb, tab, rows, g_out, g_b);
      break;
    case PD_POSE_GENERALIZED_FORCE:
      if (out) hipLaunchKernelGGL(k_generalized_force_fwd, grid, block, 0, st, count, nb, tab, rows, out);
      else hipLaunchKernelGGL(k_generalized_force_vjp, grid, block, 0, st, count, nb, tab, rows, g_out, g_b);
      break;
    case PD_POSE_BODY_TWIST:
      if (out) hipLaunchKernelGGL(k_body_twist_fwd, grid, block, 0, st, count, nb, tab, rows, out);
      else hipLaunchKernelGGL(k_body_twist_vjp, grid, block, 0, st, count, nb, tab, rows, g_out, g_b);
      break;
    case PD_POSE_BODY_ACCEL:
      if (out) hipLaunchKernelGGL(k_body_accel_fwd, grid, block, 0, st, count, nb, tab, rows, out);
      else hipLaunchKernelGGL(k_body_accel_vjp, grid, block, 0, st, count, nb, tab, rows, g_out, g_b);
      break;
    case PD_POSE_MASS_INVERSE:  // (forward only: the VJP was refused above)
      hipLaunchKernelGGL(k_mass_inverse, grid, block, 0, st, count, nb, tab, rows, out);
      break;
    case PD_POSE_MASS_MATRIX:
      if (out) hipLaunchKernelGGL(k_mass_matrix, grid, block, 0, st, count, nb, tab, rows, out);
      else hipLaunchKernelGGL(k_mass_matrix_vjp, grid, block, 0, st, count, nb, tab, rows, g_out, g_b);
      break;
    default:
      if (out) hipLaunchKernelGGL(k_contact_state_fwd, grid, block, 0, st, count, nb, tab, rows, out);
      else hipLaunchKernelGGL(k_contact_state_vjp, grid, block, 0, st, count, nb, tab, rows, g_out, g_b);
  }
  if (hipGetLastError() == hipSuccess) return 0;
  pd_set_error("pd_pose_op: the kernel launch failed");
  return 2;
}

int pose_dispatch(int op, int n, const float *a, int a_bcast, const float *b, float *out, const float *g_out, float *g_a, float *g_b, void *stream,
                  bool vjp) {  // vjp: which entry calls (at n = 0 every pointer may be NULL)
  if (n < 0 || op < 0 || (op > PD_POSE_JOINT_COORDS && op != PD_POSE_CENTROIDAL && op != PD_POSE_CONTACT_STATE && op != PD_POSE_JOINT_WRENCH &&
                         op != PD_POSE_GENERALIZED_FORCE && op != PD_POSE_BODY_TWIST && op != PD_POSE_BODY_ACCEL && op != PD_POSE_MASS_INVERSE &&
                         op != PD_POSE_MASS_MATRIX))  // (codes 7, 8, 10, 12, 14, 16, 18, 20 and 22 are not assigned: include/ppr_diffphys.h)
    return pd_set_error("pd_pose_op: n < 0 or an unknown op");
  for (const TabledOp &T : TABLED)
    if (op == T.op) return launch_tabled(T, n, a, a_bcast, b, out, g_out, g_a, g_b, (hipStream_t)stream, vjp);
  const bool project = op >= PD_POSE_PROJECT;
  if (project && (a_bcast < 0 || (a_bcast > 0 && n % a_bcast != 0)))  // before the n == 0 return: a bad group size is refused at every n
    return pd_set_error("pd_pose_op: n % g != 0 -- the element count must be a multiple of the camera group size a_broadcast");
  if (n == 0) return 0;
  if (!a || !b) return pd_set_error("pd_pose_op: a NULL operand");
  hipStream_t st = (hipStream_t)stream;
  switch (op) {
    case OP_COMPOSE_DELTA: return launch_pose<OP_COMPOSE_DELTA>(n, a, a_bcast, b, out, g_out, g_a, g_b, st);
    case OP_ROTATE_FRAME: return launch_pose<OP_ROTATE_FRAME>(n, a, a_bcast, b, out, g_out, g_a, g_b, st);
    case OP_ROTATE_VEL: return launch_pose<OP_ROTATE_VEL>(n, a, a_bcast, b, out, g_out, g_a, g_b, st);
    case OP_PROJECT: return launch_pose<OP_PROJECT>(n, a, a_bcast, b, out, g_out, g_a, g_b, st);
    default: return launch_pose<OP_PROJECT_POINT>(n, a, a_bcast, b, out, g_out, g_a, g_b, st);
  }
}

// Column sums of a row-major [n][k] matrix -- the bias gradient of a linear layer (n samples) and the gradient of a broadcast operand.
// Two fixed-order stages, no atomics: workgroup (column slab of 32, row slice s of PD_COLSUM_SLICES) -- thread (phase p = tid / 32, column
// c = tid % 32) adds the rows p, p + 8, ... of its slice (a 128-byte coalesced read per row and phase, four independent partial sums per
// thread to keep loads in flight), the 8 phases are added in LDS in the order 0 .. 7 -> ws[s][col]; the second launch adds the slices in the
// order 0 .. S-1.  The same bits every time, eagerly and inside a captured HIP graph (torch's multi-block sum(0) re-arms a semaphore with a
// memset that a graph replay does not re-execute on this stack).  Small n: one slice, straight to out, one launch.
__global__ __launch_bounds__(256) void k_colsum(int n, int k, int rows_per_slice, const float *__restrict__ x, float *__restrict__ dst) {
  __shared__ float part[8][33];
  const int c = threadIdx.x & 31, p = threadIdx.x >> 5, col = blockIdx.x * 32 + c;
  const int r0 = blockIdx.y * rows_per_slice, r1 = min(n, r0 + rows_per_slice);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (col < k) {
    const float *xc = x + col;
    int r = r0 + p;
    for (; r + 24 < r1; r += 32) {
      s0 += xc[(size_t)r * k]; s1 += xc[(size_t)(r + 8) * k]; s2 += xc[(size_t)(r + 16) * k]; s3 += xc[(size_t)(r + 24) * k];
    }
    for (; r < r1; r += 8) s0 += xc[(size_t)r * k];
  }
  part[p][c] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (p == 0 && col < k) {
    float t = part[0][c];
#pragma unroll
    for (int q = 1; q < 8; ++q) t += part[q][c];
    dst[(size_t)blockIdx.y * k + col] = t;
  }
}
__global__ __launch_bounds__(64) void k_colsum_final(int k, int slices, const float *__restrict__ ws, float *__restrict__ out) {
  const int col = blockIdx.x * 64 + threadIdx.x;
  if (col >= k) return;
  float v[PD_COLSUM_SLICES];   // all the slices' loads in flight at once (32 dependent round trips otherwise: 7 us for 32 KB), then the fixed order
#pragma unroll
  for (int s = 0; s < PD_COLSUM_SLICES; ++s) v[s] = s < slices ? ws[(size_t)s * k + col] : 0.0f;
  float t = v[0];
#pragma unroll
  for (int s = 1; s < PD_COLSUM_SLICES; ++s) t = s < slices ? t + v[s] : t;
  out[col] = t;
}

}  // namespace

extern "C" int pd_colsum(int n, int k, const float *x_dev, float *out_dev, float *ws_dev, void *stream) {
  if (n < 0 || k < 0) return 1;
  if (k == 0) return 0;
  if (!out_dev || (n > 0 && !x_dev)) return 1;
  hipStream_t st = (hipStream_t)stream;
  const unsigned slabs = (unsigned)((k + 31) / 32);
  if (n <= 1024 || !ws_dev) {  // one slice: straight to out
    hipLaunchKernelGGL(k_colsum, dim3(slabs, 1), dim3(256), 0, st, n, k, n > 0 ? n : 1, x_dev, out_dev);
    return hipGetLastError() == hipSuccess ? 0 : 2;
  }
  const int rows = (((n + PD_COLSUM_SLICES - 1) / PD_COLSUM_SLICES) + 7) & ~7;   // a multiple of the 8 row phases
  const int slices = (n + rows - 1) / rows;
  hipLaunchKernelGGL(k_colsum, dim3(slabs, (unsigned)slices), dim3(256), 0, st, n, k, rows, x_dev, ws_dev);
  hipLaunchKernelGGL(k_colsum_final, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, st, k, slices, ws_dev, out_dev);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

extern "C" int pd_pose_op(int op, int n, const float *a_dev, int a_broadcast, const float *b_dev, float *out_dev, void *stream) {
  if (n > 0 && !out_dev) return pd_set_error("pd_pose_op: out_dev is NULL");
  return pose_dispatch(op, n, a_dev, a_broadcast, b_dev, out_dev, nullptr, nullptr, nullptr, stream, false);
}

extern "C" int pd_pose_op_vjp(int op, int n, const float *a_dev, int a_broadcast, const float *b_dev, const float *g_out_dev, float *g_a_dev,
                              float *g_b_dev, void *stream) {
  if (n > 0 && (!g_out_dev || (!g_a_dev && !g_b_dev))) return pd_set_error("pd_pose_op_vjp: g_out_dev is NULL, or both g_a_dev and g_b_dev");
  return pose_dispatch(op, n, a_dev, a_broadcast, b_dev, nullptr, g_out_dev, g_a_dev, g_b_dev, stream, true);
}

extern "C" int pd_foot_height(int n, int nb, int nc, const float *body_q_dev, const int *c_body_dev, const float *c_point_dev,
                              const float *c_dist_dev, float *height_dev, int *arg_dev, void *stream) {
  if (n < 0 || nb <= 0 || nc <= 0) return 1;
  if (n == 0) return 0;
  if (!body_q_dev || !c_body_dev || !c_point_dev || !c_dist_dev || !height_dev || !arg_dev) return 1;
  hipLaunchKernelGGL(k_foot_height, dim3(n), dim3(256), 0, (hipStream_t)stream, nb, nc, body_q_dev, c_body_dev, c_point_dev, c_dist_dev,
                     height_dev, arg_dev);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

extern "C" int pd_foot_height_vjp(int n, int nb, const float *body_q_dev, const int *c_body_dev, const float *c_point_dev, const int *arg_dev,
                                  const float *g_height_dev, float *g_body_q_dev, void *stream) {
  if (n < 0 || nb <= 0) return 1;
  if (n == 0) return 0;
  if (!body_q_dev || !c_body_dev || !c_point_dev || !arg_dev || !g_height_dev || !g_body_q_dev) return 1;
  const long long total = (long long)n * nb;
  hipLaunchKernelGGL(k_foot_height_vjp, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, nb, body_q_dev, c_body_dev,
                     c_point_dev, arg_dev, g_height_dev, g_body_q_dev);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
