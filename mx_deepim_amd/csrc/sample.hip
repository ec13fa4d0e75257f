// R-group: the random draws of the training loader, on the device.
//   Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) as a counter-based generator
//   the rendered-pose rule of toolkit/LM6d_1_gen_rendered_pose.py:80-107 on top of it
//   the draws of lib/utils/mask_dilate.py:19-47
//   the background draws of lib/utils/image.py:97-116
//   the synthetic observed poses of toolkit/LM6d_ds_0_gen_observed_poses.py:200-250 and the lights of
//   toolkit/LM6d_ds_1_gen_observed.py:116-144
//
// Every draw is a pure function of (seed, draw id, attempt, stream): key = (seed lo, seed hi), counter = (id lo, id hi, attempt,
// stream). Streams 0 and 1 are the two blocks of a pose draw, stream 2 is the mask-dilate draw, stream 3 the background draw,
// streams 4 and 5 the quaternion and translation blocks of an observed-pose draw, stream 6 the light draw, streams 7 and 8 the
// placement and rotation blocks of a scene's occluders (attempt = the slot; attempt 0 of stream 7 is their count).
// Nothing depends on the batch size, on a pair's position in the batch or on the order of launches.
//
// The kernels run one thread per pair; every array below is indexed by constants after unrolling, so nothing lives in
// private memory. Arithmetic is float64 throughout (full rate on CDNA4, a few hundred flops per candidate).
#include "common.h"
#include "euler_f64.h"

namespace {

struct Philox4 { unsigned int w[4]; };

__device__ __forceinline__ Philox4 philox4x32_10(unsigned int c0, unsigned int c1, unsigned int c2, unsigned int c3,
                                                 unsigned int k0, unsigned int k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c1 ^ k0;
    const unsigned int n2 = (unsigned int)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned int)p1;
    c3 = (unsigned int)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  Philox4 o;
  o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
  return o;
}

__device__ __forceinline__ Philox4 philox_draw(unsigned long long seed, unsigned long long id, unsigned int attempt,
                                               unsigned int stream) {
  return philox4x32_10((unsigned int)id, (unsigned int)(id >> 32), attempt, stream, (unsigned int)seed,
                       (unsigned int)(seed >> 32));
}

// a 32-bit word as a uniform strictly inside (0,1): (x + 0.5) 2^-32, exact in double
__device__ __forceinline__ double word_uniform(unsigned int x) { return ((double)x + 0.5) * 2.3283064365386963e-10; }

// Box-Muller in double: two words -> two independent standard normals
__device__ __forceinline__ void box_muller(unsigned int a, unsigned int b, double& z0, double& z1) {
  const double r = sqrt(-2.0 * log(word_uniform(a)));
  const double t = 6.283185307179586 * word_uniform(b);
  z0 = r * cos(t);
  z1 = r * sin(t);
}

// the six normals of one candidate: block 0 (stream 0) gives z0..z3, block 1 (stream 1) z4, z5 from its first two words
__device__ __forceinline__ void pose_normals(unsigned long long seed, unsigned long long id, unsigned int attempt, double* z) {
  const Philox4 a = philox_draw(seed, id, attempt, 0u);
  const Philox4 b = philox_draw(seed, id, attempt, 1u);
  box_muller(a.w[0], a.w[1], z[0], z[1]);
  box_muller(a.w[2], a.w[3], z[2], z[3]);
  box_muller(b.w[0], b.w[1], z[4], z[5]);
}

// a word mapped to [0, n): (x n) >> 32. The bias of any value's probability is at most n 2^-32.
__device__ __forceinline__ int word_below(unsigned int x, int n) {
  return (int)(((unsigned long long)x * (unsigned long long)(unsigned int)n) >> 32);
}

struct PoseNoise {
  Mat3 K;
  float angle_std, angle_max, x_std, y_std, z_std;   // degrees, degrees, metres
  float border;
  int width, height;
};

// One candidate of LM6d_1_gen_rendered_pose.py:86-97 from given normals, in float64:
//   tgt_euler = mat2euler(R_src) + z[0:3] angle_std pi/180, tgt_trans = T_src + z[3:6] (x_std, y_std, z_std), R_tgt = euler2mat
//   r_dist = angle of R_src^T R_tgt in degrees, as atan2(|antisymmetric part| / 2, (trace - 1) / 2): calc_rt_dist_m takes
//   ||logm||_F / sqrt 2, the same value for a rotation; this form keeps its digits at small angles
//   (cx, cy) = projection of tgt_trans through K
//   accept iff r_dist <= angle_max and border < cx < W - border and border < cy < H - border and tgt_trans.z > 0
// The z > 0 clause is not the reference's, which divides by z unguarded.
// pose: the candidate [R | t] in double (12); stat: r_dist, cx, cy. Returns the accept flag.
__device__ __forceinline__ bool pose_perturb_one(const float* src, const double* z, const PoseNoise& p, double* pose, double* stat) {
  double Rs[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Rs[i * 3 + j] = (double)src[i * 4 + j];
  double e[3];
  mat2euler_sxyz_f64(Rs, e);
  const double scale = (double)p.angle_std / 180.0 * 3.141592653589793;
  double Rt[9];
  euler2mat_sxyz_f64(e[0] + z[0] * scale, e[1] + z[1] * scale, e[2] + z[2] * scale, Rt);
  const double tx = (double)src[3] + z[3] * (double)p.x_std;
  const double ty = (double)src[7] + z[4] * (double)p.y_std;
  const double tz = (double)src[11] + z[5] * (double)p.z_std;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) pose[i * 4 + j] = Rt[i * 3 + j];
  pose[3] = tx; pose[7] = ty; pose[11] = tz;
  // M = R_src^T R_tgt
  double M[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[i * 3 + j] = (Rs[i] * Rt[j] + Rs[3 + i] * Rt[3 + j]) + Rs[6 + i] * Rt[6 + j];
  const double c = ((M[0] + M[4] + M[8]) - 1.0) * 0.5;
  const double sx = (M[7] - M[5]) * 0.5, sy = (M[2] - M[6]) * 0.5, sz = (M[3] - M[1]) * 0.5;
  const double r_dist = atan2(sqrt((sx * sx + sy * sy) + sz * sz), c) / 3.141592653589793 * 180.0;
  const double px = ((double)p.K.v[0] * tx + (double)p.K.v[1] * ty) + (double)p.K.v[2] * tz;
  const double py = ((double)p.K.v[3] * tx + (double)p.K.v[4] * ty) + (double)p.K.v[5] * tz;
  const double pz = ((double)p.K.v[6] * tx + (double)p.K.v[7] * ty) + (double)p.K.v[8] * tz;
  const double cx = px / pz, cy = py / pz;
  stat[0] = r_dist; stat[1] = cx; stat[2] = cy;
  const double lo = (double)p.border;
  return r_dist <= (double)p.angle_max && lo < cx && cx < (double)p.width - lo && lo < cy && cy < (double)p.height - lo &&
         tz > 0.0;
}

__global__ __launch_bounds__(256) void philox_selfcheck_kernel(unsigned int* __restrict__ out, const unsigned int* __restrict__ ctr,
                                                               const unsigned int* __restrict__ key, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const Philox4 o = philox4x32_10(ctr[i * 4], ctr[i * 4 + 1], ctr[i * 4 + 2], ctr[i * 4 + 3], key[i * 2], key[i * 2 + 1]);
#pragma unroll
  for (int k = 0; k < 4; ++k) out[i * 4 + k] = o.w[k];
}

__global__ __launch_bounds__(256) void pose_perturb_kernel(float* __restrict__ pose_out, double* __restrict__ stat_out,
                                                           const float* __restrict__ pose_src, const double* __restrict__ normals,
                                                           PoseNoise p, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float P[12];
  double z[6], pose[12], stat[3];
#pragma unroll
  for (int i = 0; i < 12; ++i) P[i] = pose_src[(long)b * 12 + i];
#pragma unroll
  for (int i = 0; i < 6; ++i) z[i] = normals[(long)b * 6 + i];
  const bool ok = pose_perturb_one(P, z, p, pose, stat);
#pragma unroll
  for (int i = 0; i < 12; ++i) pose_out[(long)b * 12 + i] = (float)pose[i];
  if (stat_out) {
#pragma unroll
    for (int i = 0; i < 3; ++i) stat_out[(long)b * 4 + i] = stat[i];
    stat_out[(long)b * 4 + 3] = ok ? 1.0 : 0.0;
  }
}

// The attempt loop of LM6d_1_gen_rendered_pose.py:86-110 with a bound: the first accepted candidate of attempts
// 0 .. max_attempts-1, attempts[b] = candidates drawn (1 .. max_attempts); none accepted: pose_src unchanged, attempts[b] = 0
// and zeros in normals_out (the reference loops for ever there).
__global__ __launch_bounds__(256) void sample_rendered_poses_kernel(float* __restrict__ pose_out, int* __restrict__ attempts,
                                                                    double* __restrict__ normals_out,
                                                                    const float* __restrict__ pose_src, PoseNoise p, int max_attempts,
                                                                    unsigned long long seed, unsigned long long draw_base,
                                                                    const unsigned long long* __restrict__ draw_ids, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const unsigned long long id = draw_ids ? draw_ids[b] : draw_base + (unsigned long long)b;
  float P[12], out[12];
  double zk[6];
#pragma unroll
  for (int i = 0; i < 12; ++i) { P[i] = pose_src[(long)b * 12 + i]; out[i] = P[i]; }
#pragma unroll
  for (int i = 0; i < 6; ++i) zk[i] = 0.0;
  int used = 0;
  for (int a = 0; a < max_attempts; ++a) {
    double z[6], pose[12], stat[3];
    pose_normals(seed, id, (unsigned int)a, z);
    if (pose_perturb_one(P, z, p, pose, stat)) {
#pragma unroll
      for (int i = 0; i < 12; ++i) out[i] = (float)pose[i];
#pragma unroll
      for (int i = 0; i < 6; ++i) zk[i] = z[i];
      used = a + 1;
      break;
    }
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) pose_out[(long)b * 12 + i] = out[i];
  attempts[b] = used;
  if (normals_out) {
#pragma unroll
    for (int i = 0; i < 6; ++i) normals_out[(long)b * 6 + i] = zk[i];
  }
}

// mask_dilate.py:19-47's draws from stream 2: word 0 of the call with attempt 0 is the direction in [0,10); words 1..3 of that
// call and word 0 of the call with attempt 1 are the four sides' randint(max_thickness) + 1, in the order of the file's four
// blocks; a side is 0 where the file skips it for the direction (:22 0,1,4; :28 1,2,5; :34 2,3,6; :40 0,3,7).
__global__ __launch_bounds__(256) void sample_mask_dilate_kernel(int* __restrict__ thickness, int max_thickness,
                                                                 unsigned long long seed, unsigned long long draw_base,
                                                                 const unsigned long long* __restrict__ draw_ids, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const unsigned long long id = draw_ids ? draw_ids[b] : draw_base + (unsigned long long)b;
  const Philox4 c0 = philox_draw(seed, id, 0u, 2u);
  const Philox4 c1 = philox_draw(seed, id, 1u, 2u);
  const int direction = word_below(c0.w[0], 10);
  const unsigned int bit = 1u << direction;
  int4 t;
  t.x = (bit & 0x013u) ? 0 : word_below(c0.w[1], max_thickness) + 1;
  t.y = (bit & 0x026u) ? 0 : word_below(c0.w[2], max_thickness) + 1;
  t.z = (bit & 0x04Cu) ? 0 : word_below(c0.w[3], max_thickness) + 1;
  t.w = (bit & 0x089u) ? 0 : word_below(c1.w[0], max_thickness) + 1;
  reinterpret_cast<int4*>(thickness)[b] = t;
}

// The background draws of image.py:97-116 from stream 3, attempt 0: word 0 as a uniform is the np.random.rand() held against
// TRAIN.REPLACE_OBSERVED_BG_RATIO (:99), which a data_syn frame (`always`) does not need (:98); word 1 is random.randint's
// choice among the pool's images (:113). Both are drawn for every pair, used or not.
__global__ __launch_bounds__(256) void sample_backgrounds_kernel(int* __restrict__ use_bg, int* __restrict__ bg_index,
                                                                 const int* __restrict__ always, double ratio, int pool_size,
                                                                 unsigned long long seed, unsigned long long draw_base,
                                                                 const unsigned long long* __restrict__ draw_ids, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const unsigned long long id = draw_ids ? draw_ids[b] : draw_base + (unsigned long long)b;
  const Philox4 c = philox_draw(seed, id, 0u, 3u);
  use_bg[b] = ((always && always[b] != 0) || word_uniform(c.w[0]) < ratio) ? 1 : 0;
  bg_index[b] = word_below(c.w[1], pool_size);
}

// totals[0] += B, totals[1] += sum of attempts, totals[2] += pairs with attempts == 0. One block: integer sums, any order.
__global__ __launch_bounds__(256) void sample_stats_kernel(unsigned long long* __restrict__ totals, const int* __restrict__ attempts,
                                                           int B) {
  __shared__ unsigned long long red[4][2];
  unsigned long long sum = 0, zero = 0;
  for (int b = threadIdx.x; b < B; b += 256) {
    const int a = attempts[b];
    sum += (unsigned long long)a;
    zero += a == 0 ? 1ull : 0ull;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_xor(sum, off, 64);
    zero += __shfl_xor(zero, off, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[wave][0] = sum; red[wave][1] = zero; }
  __syncthreads();
  if (threadIdx.x == 0) {
    totals[0] += (unsigned long long)B;
    totals[1] += (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    totals[2] += (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
  }
}

// ---- synthetic observed frames: the pose of LM6d_ds_0_gen_observed_poses.py and the light of LM6d_ds_1_gen_observed.py

constexpr int OBS_ROW = 22;      // a class's row: trans_mean[3], trans_std[3], pz_mean[3], angle_max (degrees), fallback pose [12]

struct ObservedRule {
  Mat3 K;
  float border;
  int width, height;
};

// the seven normals of one candidate: stream 4 gives z0..z3 (the quaternion), stream 5 z4..z6 (the translation; the second
// normal of its second pair is not used)
__device__ __forceinline__ void observed_normals(unsigned long long seed, unsigned long long id, unsigned int attempt, double* z) {
  const Philox4 a = philox_draw(seed, id, attempt, 4u);
  const Philox4 b = philox_draw(seed, id, attempt, 5u);
  double unused;
  box_muller(a.w[0], a.w[1], z[0], z[1]);
  box_muller(a.w[2], a.w[3], z[2], z[3]);
  box_muller(b.w[0], b.w[1], z[4], z[5]);
  box_muller(b.w[2], b.w[3], z[6], unused);
}

// Four normals as a rotation: the quaternion z / |z|, negated if w < 0, through RT_transform.quat2mat in its expression order.
__device__ __forceinline__ void normals_to_rotation(const double* z, double* R) {
  const double n = sqrt(((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2]) + z[3] * z[3]);
  double w = z[0] / n, x = z[1] / n, y = z[2] / n, q = z[3] / n;
  if (w < 0.0) { w = -w; x = -x; y = -y; q = -q; }
  const double Nq = ((w * w + x * x) + y * y) + q * q;
  R[0] = 1.0; R[1] = 0.0; R[2] = 0.0; R[3] = 0.0; R[4] = 1.0; R[5] = 0.0; R[6] = 0.0; R[7] = 0.0; R[8] = 1.0;
  if (!(Nq < 2.220446049250313e-16)) {
    const double s = 2.0 / Nq;
    const double X = x * s, Y = y * s, Z = q * s;
    const double wX = w * X, wY = w * Y, wZ = w * Z;
    const double xX = x * X, xY = x * Y, xZ = x * Z;
    const double yY = y * Y, yZ = y * Z, zZ = q * Z;
    R[0] = 1.0 - (yY + zZ); R[1] = xY - wZ; R[2] = xZ + wY;
    R[3] = xY + wZ; R[4] = 1.0 - (xX + zZ); R[5] = yZ - wX;
    R[6] = xZ - wY; R[7] = yZ + wX; R[8] = 1.0 - (xX + yY);
  }
}

// One candidate of LM6d_ds_0_gen_observed_poses.py:203-220 from given normals, in float64:
//   tgt_quat = z[0:4] / |z[0:4]|, negated if w < 0      tgt_trans = trans_mean + z[4:7] trans_std (np.random.normal(mean, std))
//   R = quat2mat(tgt_quat) in the expression order of RT_transform.quat2mat
//   deg = angle(R e_z, pz_mean) as :74-78: arccos(clip(u.v / (|u| |v|), -1, 1)) in degrees
//   (cx, cy) = the projection of tgt_trans through K
//   accept iff deg <= angle_max and border < cx < W - border and border < cy < H - border and tgt_trans.z > 0
// The z > 0 clause is not the reference's, which divides by z unguarded (as in pose_perturb_one).
// row: the class's table row; pose: the candidate [R | t] in double (12); stat: deg, cx, cy. Returns the accept flag.
__device__ __forceinline__ bool observed_pose_one(const double* __restrict__ row, const double* z, const ObservedRule& p, double* pose,
                                                  double* stat) {
  double R[9];
  normals_to_rotation(z, R);
  const double tx = row[0] + z[4] * row[3];
  const double ty = row[1] + z[5] * row[4];
  const double tz = row[2] + z[6] * row[5];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) pose[i * 4 + j] = R[i * 3 + j];
  pose[3] = tx; pose[7] = ty; pose[11] = tz;
  const double ux = R[2], uy = R[5], uz = R[8], vx = row[6], vy = row[7], vz = row[8];
  const double c = ((ux * vx + uy * vy) + uz * vz) / (sqrt((ux * ux + uy * uy) + uz * uz) * sqrt((vx * vx + vy * vy) + vz * vz));
  const double deg = acos(fmin(fmax(c, -1.0), 1.0)) / 3.141592653589793 * 180.0;      // a NaN (zero pz_mean) stays NaN: rejected
  const double px = ((double)p.K.v[0] * tx + (double)p.K.v[1] * ty) + (double)p.K.v[2] * tz;
  const double py = ((double)p.K.v[3] * tx + (double)p.K.v[4] * ty) + (double)p.K.v[5] * tz;
  const double pz = ((double)p.K.v[6] * tx + (double)p.K.v[7] * ty) + (double)p.K.v[8] * tz;
  const double cx = px / pz, cy = py / pz;
  stat[0] = c == c ? deg : c; stat[1] = cx; stat[2] = cy;
  const double lo = (double)p.border;
  return c == c && deg <= row[9] && lo < cx && cx < (double)p.width - lo && lo < cy && cy < (double)p.height - lo && tz > 0.0;
}

// The candidate of GIVEN normals for every pair, accepted or not (the replay of a golden run). A class id outside the table:
// zeros in pose_out and stat_out.
__global__ __launch_bounds__(256) void observed_pose_kernel(float* __restrict__ pose_out, double* __restrict__ stat_out,
                                                            const int* __restrict__ class_index, const double* __restrict__ table,
                                                            int n_classes, const double* __restrict__ normals, ObservedRule p, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int cls = class_index[b];
  double z[7], pose[12], stat[3];
#pragma unroll
  for (int i = 0; i < 12; ++i) pose[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) stat[i] = 0.0;
  bool ok = false;
  if ((unsigned)cls < (unsigned)n_classes) {
#pragma unroll
    for (int i = 0; i < 7; ++i) z[i] = normals[(long)b * 7 + i];
    ok = observed_pose_one(table + (long)cls * OBS_ROW, z, p, pose, stat);
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) pose_out[(long)b * 12 + i] = (float)pose[i];
  if (stat_out) {
#pragma unroll
    for (int i = 0; i < 3; ++i) stat_out[(long)b * 4 + i] = stat[i];
    stat_out[(long)b * 4 + 3] = ok ? 1.0 : 0.0;
  }
}

// The attempt loop of LM6d_ds_0_gen_observed_poses.py:203-236 with a bound: the first accepted candidate of attempts
// 0 .. max_attempts-1, attempts[b] = candidates drawn (1 .. max_attempts). None accepted: the class's fallback pose,
// attempts[b] = 0, zeros in normals_out and stat_out (the reference loops for ever there). A class id outside the table:
// an all-zero pose and attempts[b] = -1; the table is not read.
__global__ __launch_bounds__(256) void sample_observed_poses_kernel(float* __restrict__ pose_out, int* __restrict__ attempts,
                                                                    double* __restrict__ normals_out, double* __restrict__ stat_out,
                                                                    const int* __restrict__ class_index,
                                                                    const double* __restrict__ table, int n_classes, ObservedRule p,
                                                                    int max_attempts, unsigned long long seed,
                                                                    unsigned long long draw_base,
                                                                    const unsigned long long* __restrict__ draw_ids, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const unsigned long long id = draw_ids ? draw_ids[b] : draw_base + (unsigned long long)b;
  const int cls = class_index[b];
  const bool known = (unsigned)cls < (unsigned)n_classes;
  const double* __restrict__ row = table + (long)(known ? cls : 0) * OBS_ROW;
  float out[12];
  double zk[7], sk[4];
#pragma unroll
  for (int i = 0; i < 12; ++i) out[i] = known ? (float)row[10 + i] : 0.f;
#pragma unroll
  for (int i = 0; i < 7; ++i) zk[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) sk[i] = 0.0;
  int used = known ? 0 : -1;
  for (int a = 0; known && a < max_attempts; ++a) {
    double z[7], pose[12], stat[3];
    observed_normals(seed, id, (unsigned int)a, z);
    if (observed_pose_one(row, z, p, pose, stat)) {
#pragma unroll
      for (int i = 0; i < 12; ++i) out[i] = (float)pose[i];
#pragma unroll
      for (int i = 0; i < 7; ++i) zk[i] = z[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) sk[i] = stat[i];
      sk[3] = 1.0;
      used = a + 1;
      break;
    }
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) pose_out[(long)b * 12 + i] = out[i];
  attempts[b] = used;
  if (normals_out) {
#pragma unroll
    for (int i = 0; i < 7; ++i) normals_out[(long)b * 7 + i] = zk[i];
  }
  if (stat_out) {
#pragma unroll
    for (int i = 0; i < 4; ++i) stat_out[(long)b * 4 + i] = sk[i];
  }
}

// ---- occluders of a synthetic scene (ours: the reference has no generator for occluded scenes)

struct OccluderRule {
  int min_occluders, max_occluders, n_list, n_classes;
  float lateral_lo, lateral_hi, toward_lo, toward_hi;      // in diameters of the target's class
};

// The S = max_occluders + 1 slots of pair b: slot 0 is the target, copied through. Stream 7, attempt 0, word 0 -> the count n in
// [min, max] (not drawn when max_occluders = 0). Slot s = 1..n: stream 7, attempt s -> word 0 the class out of `list` (it may be
// the target's), words 1-3 as uniforms rho in lateral, phi in [0, 2 pi), tau in toward: t = t_target + d (rho cos phi,
// rho sin phi, -tau), d = diameters[target class] (0 for a class id outside the table); stream 8, attempt s -> four normals ->
// the rotation, as stream 4's. Slots beyond n, and an occluder behind the camera (t_z <= 0): class -1, a zero pose.
__global__ __launch_bounds__(256) void sample_occluders_kernel(int* __restrict__ class_out, float* __restrict__ pose_out,
                                                               int* __restrict__ label_out, const int* __restrict__ target_class,
                                                               const float* __restrict__ target_pose, const int* __restrict__ list,
                                                               const float* __restrict__ diameters, OccluderRule p,
                                                               unsigned long long seed, unsigned long long draw_base,
                                                               const unsigned long long* __restrict__ draw_ids, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const unsigned long long id = draw_ids ? draw_ids[b] : draw_base + (unsigned long long)b;
  const int S = p.max_occluders + 1;
  const int cls = target_class[b];
  float T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = target_pose[(long)b * 12 + i];
  class_out[(long)b * S] = cls;
  label_out[(long)b * S] = 1;
#pragma unroll
  for (int i = 0; i < 12; ++i) pose_out[(long)b * S * 12 + i] = T[i];
  if (S == 1) return;
  const double d = (unsigned)cls < (unsigned)p.n_classes ? (double)diameters[cls] : 0.0;
  const int n = p.min_occluders + word_below(philox_draw(seed, id, 0u, 7u).w[0], p.max_occluders - p.min_occluders + 1);
  for (int s = 1; s < S; ++s) {
    int c = -1;
    float out[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) out[i] = 0.f;
    if (s <= n) {
      const Philox4 a = philox_draw(seed, id, (unsigned int)s, 7u);
      const Philox4 r = philox_draw(seed, id, (unsigned int)s, 8u);
      const double rho = (double)p.lateral_lo + ((double)p.lateral_hi - (double)p.lateral_lo) * word_uniform(a.w[1]);
      const double phi = 6.283185307179586 * word_uniform(a.w[2]);
      const double tau = (double)p.toward_lo + ((double)p.toward_hi - (double)p.toward_lo) * word_uniform(a.w[3]);
      const double tx = (double)T[3] + d * (rho * cos(phi));
      const double ty = (double)T[7] + d * (rho * sin(phi));
      const double tz = (double)T[11] - d * tau;
      if (tz > 0.0) {
        double z[4], R[9];
        box_muller(r.w[0], r.w[1], z[0], z[1]);
        box_muller(r.w[2], r.w[3], z[2], z[3]);
        normals_to_rotation(z, R);
        c = list[word_below(a.w[0], p.n_list)];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) out[i * 4 + j] = (float)R[i * 3 + j];
        out[3] = (float)tx; out[7] = (float)ty; out[11] = (float)tz;
      }
    }
    class_out[(long)b * S + s] = c;
    label_out[(long)b * S + s] = s + 1;
#pragma unroll
    for (int i = 0; i < 12; ++i) pose_out[((long)b * S + s) * 12 + i] = out[i];
  }
}

struct Ratios { float v[8]; };

// The light of LM6d_ds_1_gen_observed.py:116-144 for the frame whose running index is the draw id:
//   light_offset = 0.5 x row (id mod 6) of [1,0,1], [1,1,1], [0,1,1], [-1,1,1], [-1,0,1], [0,0,1]   (:117-131; the absolute
//       position of :133-135 adds (t_x, -t_y, -t_z), which the lit draw does itself)
//   stream 6, attempt 0: words 0-2 -> intensity[c] = 0.9 + 0.2 u (np.random.uniform(0.9, 1.1), :139); word 3 -> one of the seven
//       colour rows [0,0,1] .. [1,1,1] (:138,140), row k being the bits of k + 1; light_intensity = colour * intensity (:141)
//   stream 6, attempt 1: word 0 -> one of the n_ratios brightness ratios (:144)
__global__ __launch_bounds__(256) void sample_lights_kernel(float* __restrict__ light_offset, float* __restrict__ light_intensity,
                                                            float* __restrict__ brightness_ratio, Ratios ratios, int n_ratios,
                                                            unsigned long long seed, unsigned long long draw_base,
                                                            const unsigned long long* __restrict__ draw_ids, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const unsigned long long id = draw_ids ? draw_ids[b] : draw_base + (unsigned long long)b;
  const int m = (int)(id % 6ull);
  light_offset[(long)b * 3 + 0] = 0.5f * (m < 2 ? 1.f : (m == 2 || m == 5) ? 0.f : -1.f);
  light_offset[(long)b * 3 + 1] = 0.5f * ((m >= 1 && m <= 3) ? 1.f : 0.f);
  light_offset[(long)b * 3 + 2] = 0.5f;
  const Philox4 c0 = philox_draw(seed, id, 0u, 6u);
  const Philox4 c1 = philox_draw(seed, id, 1u, 6u);
  const int colour = word_below(c0.w[3], 7) + 1;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double inten = 0.9 + 0.2 * word_uniform(c0.w[c]);
    light_intensity[(long)b * 3 + c] = ((colour >> (2 - c)) & 1) ? (float)inten : 0.f;
  }
  const int k = word_below(c1.w[0], n_ratios);
  float r = ratios.v[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) r = k == i ? ratios.v[i] : r;
  brightness_ratio[b] = r;
}

int observed_rule_from(ObservedRule* p, const float* K_host, int width, int height, float border) {
  DI_REQUIRE(K_host, "observed poses: K is a host array, not NULL");
  for (int i = 0; i < 9; ++i) p->K.v[i] = K_host[i];
  DI_REQUIRE(width > 0 && height > 0, "observed poses: width and height must be positive");
  p->border = border; p->width = width; p->height = height;
  return 0;
}

int pose_noise_from(PoseNoise* p, const float* K_host, const float* noise_host, int width, int height, float border) {
  DI_REQUIRE(K_host && noise_host, "pose sampler: K and noise are host arrays, not NULL");
  for (int i = 0; i < 9; ++i) p->K.v[i] = K_host[i];
  p->angle_std = noise_host[0]; p->angle_max = noise_host[1];
  p->x_std = noise_host[2]; p->y_std = noise_host[3]; p->z_std = noise_host[4];
  DI_REQUIRE(p->angle_std >= 0.f && p->x_std >= 0.f && p->y_std >= 0.f && p->z_std >= 0.f,
             "pose sampler: the standard deviations must be >= 0");
  DI_REQUIRE(width > 0 && height > 0, "pose sampler: width and height must be positive");
  p->border = border; p->width = width; p->height = height;
  return 0;
}

}  // namespace

extern "C" int deepim_selfcheck_philox(deepim_ctx* ctx, unsigned int* out, const unsigned int* ctr, const unsigned int* key, int n) {
  DI_DEVICE(ctx);
  DI_REQUIRE(n >= 0, "selfcheck_philox: n must be >= 0");
  if (n == 0) return 0;
  DI_REQUIRE(out && ctr && key, "selfcheck_philox: NULL argument");
  hipLaunchKernelGGL(philox_selfcheck_kernel, dim3(di_div_up(n, 256)), dim3(256), 0, ctx->stream, out, ctr, key, n);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_pose_perturb(deepim_ctx* ctx, float* pose_out, double* stat_out, const float* pose_src, const double* normals,
                                   const float* K, const float* noise, int width, int height, float border, int B) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0, "pose_perturb: B must be >= 0");
  PoseNoise p;
  if (pose_noise_from(&p, K, noise, width, height, border)) return -1;
  if (B == 0) return 0;
  DI_REQUIRE(pose_out && pose_src && normals, "pose_perturb: NULL argument");
  hipLaunchKernelGGL(pose_perturb_kernel, dim3(di_div_up(B, 256)), dim3(256), 0, ctx->stream, pose_out, stat_out, pose_src, normals,
                     p, B);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_sample_rendered_poses(deepim_ctx* ctx, float* pose_out, int32_t* attempts, double* normals_out, const float* pose_src,
                                            const float* K, const float* noise, int width, int height, float border,
                                            int max_attempts, unsigned long long seed, unsigned long long draw_base,
                                            const unsigned long long* draw_ids, int B) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0, "sample_rendered_poses: B must be >= 0");
  DI_REQUIRE(max_attempts >= 1, "sample_rendered_poses: max_attempts must be >= 1");
  PoseNoise p;
  if (pose_noise_from(&p, K, noise, width, height, border)) return -1;
  if (B == 0) return 0;
  DI_REQUIRE(pose_out && attempts && pose_src, "sample_rendered_poses: NULL argument");
  hipLaunchKernelGGL(sample_rendered_poses_kernel, dim3(di_div_up(B, 256)), dim3(256), 0, ctx->stream, pose_out, attempts,
                     normals_out, pose_src, p, max_attempts, seed, draw_base, draw_ids, B);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_sample_mask_dilate(deepim_ctx* ctx, int32_t* thickness, int max_thickness, unsigned long long seed,
                                         unsigned long long draw_base, const unsigned long long* draw_ids, int B) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0, "sample_mask_dilate: B must be >= 0");
  DI_REQUIRE(max_thickness >= 1, "sample_mask_dilate: max_thickness must be >= 1");
  if (B == 0) return 0;
  DI_REQUIRE(thickness, "sample_mask_dilate: NULL argument");
  hipLaunchKernelGGL(sample_mask_dilate_kernel, dim3(di_div_up(B, 256)), dim3(256), 0, ctx->stream, thickness, max_thickness, seed,
                     draw_base, draw_ids, B);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_sample_backgrounds(deepim_ctx* ctx, int32_t* use_bg, int32_t* bg_index, const int32_t* always, double ratio,
                                         int pool_size, unsigned long long seed, unsigned long long draw_base,
                                         const unsigned long long* draw_ids, int B) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0, "sample_backgrounds: B must be >= 0");
  DI_REQUIRE(pool_size >= 1, "sample_backgrounds: pool_size must be >= 1");
  DI_REQUIRE(ratio >= 0.0 && ratio <= 1.0, "sample_backgrounds: ratio must lie in [0, 1]");
  if (B == 0) return 0;
  DI_REQUIRE(use_bg && bg_index, "sample_backgrounds: NULL argument");
  hipLaunchKernelGGL(sample_backgrounds_kernel, dim3(di_div_up(B, 256)), dim3(256), 0, ctx->stream, use_bg, bg_index, always, ratio,
                     pool_size, seed, draw_base, draw_ids, B);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_observed_pose_candidate(deepim_ctx* ctx, float* pose_out, double* stat_out, const int32_t* class_index,
                                              const double* table, int n_classes, const double* normals, const float* K, int width,
                                              int height, float border, int B) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0, "observed_pose_candidate: B must be >= 0");
  DI_REQUIRE(n_classes >= 1, "observed_pose_candidate: n_classes must be >= 1");
  ObservedRule p;
  if (observed_rule_from(&p, K, width, height, border)) return -1;
  if (B == 0) return 0;
  DI_REQUIRE(pose_out && class_index && table && normals, "observed_pose_candidate: NULL argument");
  hipLaunchKernelGGL(observed_pose_kernel, dim3(di_div_up(B, 256)), dim3(256), 0, ctx->stream, pose_out, stat_out,
                     (const int*)class_index, table, n_classes, normals, p, B);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_sample_observed_poses(deepim_ctx* ctx, float* pose_out, int32_t* attempts, double* normals_out, double* stat_out,
                                            const int32_t* class_index, const double* table, int n_classes, const float* K, int width,
                                            int height, float border, int max_attempts, unsigned long long seed,
                                            unsigned long long draw_base, const unsigned long long* draw_ids, int B) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0, "sample_observed_poses: B must be >= 0");
  DI_REQUIRE(max_attempts >= 1, "sample_observed_poses: max_attempts must be >= 1");
  DI_REQUIRE(n_classes >= 1, "sample_observed_poses: n_classes must be >= 1");
  ObservedRule p;
  if (observed_rule_from(&p, K, width, height, border)) return -1;
  if (B == 0) return 0;
  DI_REQUIRE(pose_out && attempts && class_index && table, "sample_observed_poses: NULL argument");
  hipLaunchKernelGGL(sample_observed_poses_kernel, dim3(di_div_up(B, 256)), dim3(256), 0, ctx->stream, pose_out, (int*)attempts,
                     normals_out, stat_out, (const int*)class_index, table, n_classes, p, max_attempts, seed, draw_base, draw_ids, B);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_sample_lights(deepim_ctx* ctx, float* light_offset, float* light_intensity, float* brightness_ratio,
                                    const float* ratios_host, int n_ratios, unsigned long long seed, unsigned long long draw_base,
                                    const unsigned long long* draw_ids, int B) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0, "sample_lights: B must be >= 0");
  DI_REQUIRE(ratios_host && n_ratios >= 1 && n_ratios <= 8, "sample_lights: 1 to 8 brightness ratios, a host array");
  Ratios r;
  for (int i = 0; i < 8; ++i) r.v[i] = i < n_ratios ? ratios_host[i] : 0.f;
  for (int i = 0; i < n_ratios; ++i) DI_REQUIRE(r.v[i] >= 0.f && r.v[i] <= 1.f, "sample_lights: brightness ratios in [0, 1]");
  if (B == 0) return 0;
  DI_REQUIRE(light_offset && light_intensity && brightness_ratio, "sample_lights: NULL argument");
  hipLaunchKernelGGL(sample_lights_kernel, dim3(di_div_up(B, 256)), dim3(256), 0, ctx->stream, light_offset, light_intensity,
                     brightness_ratio, r, n_ratios, seed, draw_base, draw_ids, B);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_sample_occluders(deepim_ctx* ctx, int32_t* class_out, float* pose_out, int32_t* label_value_out,
                                       const int32_t* target_class, const float* target_pose, const int32_t* occluder_classes,
                                       int n_occluder_classes, const float* diameters, int n_classes, int min_occluders,
                                       int max_occluders, float lateral_lo, float lateral_hi, float toward_lo, float toward_hi,
                                       unsigned long long seed, unsigned long long draw_base, const unsigned long long* draw_ids, int B) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0, "sample_occluders: B must be >= 0");
  DI_REQUIRE(min_occluders >= 0 && max_occluders >= min_occluders && max_occluders <= 7,
             "sample_occluders: 0 <= min_occluders <= max_occluders <= 7");
  DI_REQUIRE(lateral_lo >= 0.f && lateral_hi >= lateral_lo && toward_hi >= toward_lo,
             "sample_occluders: the lateral range must be 0 <= lo <= hi and the toward range lo <= hi");
  DI_REQUIRE(max_occluders == 0 || (n_occluder_classes >= 1 && n_classes >= 1), "sample_occluders: an empty class list or diameter table");
  if (B == 0) return 0;
  DI_REQUIRE(class_out && pose_out && label_value_out && target_class && target_pose, "sample_occluders: NULL argument");
  DI_REQUIRE(max_occluders == 0 || (occluder_classes && diameters), "sample_occluders: occluder_classes and diameters are required");
  const OccluderRule p = {min_occluders, max_occluders, n_occluder_classes, n_classes, lateral_lo, lateral_hi, toward_lo, toward_hi};
  hipLaunchKernelGGL(sample_occluders_kernel, dim3(di_div_up(B, 256)), dim3(256), 0, ctx->stream, (int*)class_out, pose_out,
                     (int*)label_value_out, (const int*)target_class, target_pose, (const int*)occluder_classes, diameters, p, seed,
                     draw_base, draw_ids, B);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_sample_stats_accumulate(deepim_ctx* ctx, unsigned long long* totals, const int32_t* attempts, int B) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0, "sample_stats_accumulate: B must be >= 0");
  if (B == 0) return 0;
  DI_REQUIRE(totals && attempts, "sample_stats_accumulate: NULL argument");
  hipLaunchKernelGGL(sample_stats_kernel, dim3(1), dim3(256), 0, ctx->stream, totals, attempts, B);
  DI_LAUNCH_CHECK();
  return 0;
}
