// dsr_math.h — the pose arithmetic of the ICP tracker (k_track.h), one definition for the device and the CPU.
// Upstream's ITMPose::Coerce needs sin, cos, asin and acos; the device's libm (ocml) and glibc differ in the last bits, so the
// tracker uses the project-owned forms below: double-precision series on +, -, *, / only (IEEE, correctly rounded on both
// sides), the one square root through the Ops policy (dsr_device.h DeviceOps, or a host Ops with sqrtf).  Built with
// -ffp-contract=off everywhere, so the device and a g++ build of the CPU restatement (tests/trackref) agree bit for bit.
// Plain C++ when not compiled by hipcc: tests/trackref/track_ref.cpp includes it with g++.
#pragma once

#if defined(__HIPCC__)
#define DM_HD __host__ __device__ __forceinline__
#else
#define DM_HD inline
#endif

namespace dsr_math {

// ---- transcendentals (float in, float out; <= 1 ulp from the correctly rounded value over the ranges a pose reaches, test_track_cpu.py)

// sin / cos of a float argument: Cody-Waite reduction by pi/2 in double (exact product k * PIO2_HI for |k| < 2^20), then Taylor
// series to degree 23 on |r| <= pi/4 (truncation < 1e-20)
constexpr double kPio2Hi = 1.57079632673412561417e+00;  // the first 33 bits of pi/2
constexpr double kPio2Lo = 6.07710050650619224932e-11;  // pi/2 - kPio2Hi
constexpr double kTwoOverPi = 6.36619772367581382433e-01;
constexpr double kPi = 3.14159265358979311600e+00;
constexpr double kPio2 = 1.57079632679489655800e+00;

DM_HD double sin_series(double r) {
  const double z = r * r;
  double p = -3.86817017063068413e-23;
  p = p * z + 1.95729410633912626e-20;
  p = p * z + -8.22063524662432950e-18;
  p = p * z + 2.81145725434552060e-15;
  p = p * z + -7.64716373181981641e-13;
  p = p * z + 1.60590438368216133e-10;
  p = p * z + -2.50521083854417202e-08;
  p = p * z + 2.75573192239858925e-06;
  p = p * z + -1.98412698412698413e-04;
  p = p * z + 8.33333333333333322e-03;
  p = p * z + -1.66666666666666657e-01;
  return r + r * (z * p);
}
DM_HD double cos_series(double r) {
  const double z = r * r;
  double p = -8.89679139245057408e-22;
  p = p * z + 4.11031762331216484e-19;
  p = p * z + -1.56192069685862253e-16;
  p = p * z + 4.77947733238738525e-14;
  p = p * z + -1.14707455977297245e-11;
  p = p * z + 2.08767569878681002e-09;
  p = p * z + -2.75573192239858883e-07;
  p = p * z + 2.48015873015873016e-05;
  p = p * z + -1.38888888888888894e-03;
  p = p * z + 4.16666666666666644e-02;
  p = p * z + -5.00000000000000000e-01;
  return 1.0 + z * p;
}
// quadrant k (mod 4) and the reduced argument
DM_HD double reduce_pio2(float x, int &k) {
  const double t = (double)x * kTwoOverPi;
  k = (int)(t + (t >= 0.0 ? 0.5 : -0.5));
  const double kd = (double)k;
  return ((double)x - kd * kPio2Hi) - kd * kPio2Lo;
}
DM_HD float sinf(float x) {
  int k;
  const double r = reduce_pio2(x, k);
  double v;
  switch (k & 3) {
    case 0: v = sin_series(r); break;
    case 1: v = cos_series(r); break;
    case 2: v = -sin_series(r); break;
    default: v = -cos_series(r); break;
  }
  return (float)v;
}
DM_HD float cosf(float x) {
  int k;
  const double r = reduce_pio2(x, k);
  double v;
  switch (k & 3) {
    case 0: v = cos_series(r); break;
    case 1: v = -sin_series(r); break;
    case 2: v = -cos_series(r); break;
    default: v = sin_series(r); break;
  }
  return (float)v;
}

// asin on [0, 0.5]: its Taylor series, 30 terms (the 31st is < 1e-20 at 0.5)
DM_HD double asin_series(double a) {
  const double z = a * a;
  const double c[30] = {1.00000000000000000e+00, 1.66666666666666657e-01, 7.49999999999999972e-02, 4.46428571428571438e-02,
                        3.03819444444444441e-02, 2.23721590909090919e-02, 1.73527644230769239e-02, 1.39648437500000007e-02,
                        1.15518008961397051e-02, 9.76160952919407840e-03, 8.39033580961681506e-03, 7.31252587359884545e-03,
                        6.44721031188964875e-03, 5.74003767084192359e-03, 5.15330968231990458e-03, 4.66014348691509619e-03,
                        4.24090709367936324e-03, 3.88096455883766905e-03, 3.56920539382593474e-03, 3.29705950347348488e-03,
                        3.05782164925803065e-03, 2.84617840110894206e-03, 2.65787063820729008e-03, 2.48944867824688358e-03,
                        2.33809189211197505e-03, 2.20147397371013836e-03, 2.07766103251816759e-03, 1.96503361627728369e-03,
                        1.86222640640312754e-03, 1.76808112051541830e-03};
  double p = c[29];
  for (int i = 28; i >= 0; --i) p = p * z + c[i];
  return a * p;
}
// sqrt of h = (1 - a) / 2 for a float a in [0.5, 1] (h is then a float exactly): the float root, one Newton step in double
template <class Ops>
DM_HD double half_root(float a) {
  const float h = (1.0f - a) * 0.5f;
  const double s0 = (double)Ops::sqrt(h);
  if (s0 == 0.0) return 0.0;
  return 0.5 * (s0 + (double)h / s0);
}
// asin(|x|) for |x| <= 1, in double
template <class Ops>
DM_HD double asin_abs(float x) {
  const float a = x < 0.0f ? -x : x;
  if (a <= 0.5f) return asin_series((double)a);
  return kPio2 - 2.0 * asin_series(half_root<Ops>(a));
}
template <class Ops>
DM_HD float asinf(float x) {
  if (!(x >= -1.0f && x <= 1.0f)) return (x - x) / (x - x);  // NaN, as libm
  const double v = asin_abs<Ops>(x);
  return (float)(x < 0.0f ? -v : v);
}
template <class Ops>
DM_HD float acosf(float x) {
  if (!(x >= -1.0f && x <= 1.0f)) return (x - x) / (x - x);
  if (x >= -0.5f && x <= 0.5f) return (float)(kPio2 - (x < 0.0f ? -asin_series((double)-x) : asin_series((double)x)));
  if (x > 0.5f) return (float)(2.0 * asin_series(half_root<Ops>(x)));
  return (float)(kPi - 2.0 * asin_series(half_root<Ops>(-x)));
}

// ---- ORUtils Matrix4f (column-major m[col * 4 + row]) with upstream's operation order

// Matrix4::inv: cofactor expansion on the transposed source (the engine's host m4_inv is this function)
DM_HD bool m4_inv(const float *in, float *d) {
  float t[12], s[16], det;
  for (int i = 0; i < 4; i++) { s[i] = in[i * 4]; s[i + 4] = in[i * 4 + 1]; s[i + 8] = in[i * 4 + 2]; s[i + 12] = in[i * 4 + 3]; }
  t[0] = s[10] * s[15]; t[1] = s[11] * s[14]; t[2] = s[9] * s[15]; t[3] = s[11] * s[13];
  t[4] = s[9] * s[14]; t[5] = s[10] * s[13]; t[6] = s[8] * s[15]; t[7] = s[11] * s[12];
  t[8] = s[8] * s[14]; t[9] = s[10] * s[12]; t[10] = s[8] * s[13]; t[11] = s[9] * s[12];
  d[0] = (t[0] * s[5] + t[3] * s[6] + t[4] * s[7]) - (t[1] * s[5] + t[2] * s[6] + t[5] * s[7]);
  d[1] = (t[1] * s[4] + t[6] * s[6] + t[9] * s[7]) - (t[0] * s[4] + t[7] * s[6] + t[8] * s[7]);
  d[2] = (t[2] * s[4] + t[7] * s[5] + t[10] * s[7]) - (t[3] * s[4] + t[6] * s[5] + t[11] * s[7]);
  d[3] = (t[5] * s[4] + t[8] * s[5] + t[11] * s[6]) - (t[4] * s[4] + t[9] * s[5] + t[10] * s[6]);
  d[4] = (t[1] * s[1] + t[2] * s[2] + t[5] * s[3]) - (t[0] * s[1] + t[3] * s[2] + t[4] * s[3]);
  d[5] = (t[0] * s[0] + t[7] * s[2] + t[8] * s[3]) - (t[1] * s[0] + t[6] * s[2] + t[9] * s[3]);
  d[6] = (t[3] * s[0] + t[6] * s[1] + t[11] * s[3]) - (t[2] * s[0] + t[7] * s[1] + t[10] * s[3]);
  d[7] = (t[4] * s[0] + t[9] * s[1] + t[10] * s[2]) - (t[5] * s[0] + t[8] * s[1] + t[11] * s[2]);
  t[0] = s[2] * s[7]; t[1] = s[3] * s[6]; t[2] = s[1] * s[7]; t[3] = s[3] * s[5];
  t[4] = s[1] * s[6]; t[5] = s[2] * s[5]; t[6] = s[0] * s[7]; t[7] = s[3] * s[4];
  t[8] = s[0] * s[6]; t[9] = s[2] * s[4]; t[10] = s[0] * s[5]; t[11] = s[1] * s[4];
  d[8] = (t[0] * s[13] + t[3] * s[14] + t[4] * s[15]) - (t[1] * s[13] + t[2] * s[14] + t[5] * s[15]);
  d[9] = (t[1] * s[12] + t[6] * s[14] + t[9] * s[15]) - (t[0] * s[12] + t[7] * s[14] + t[8] * s[15]);
  d[10] = (t[2] * s[12] + t[7] * s[13] + t[10] * s[15]) - (t[3] * s[12] + t[6] * s[13] + t[11] * s[15]);
  d[11] = (t[5] * s[12] + t[8] * s[13] + t[11] * s[14]) - (t[4] * s[12] + t[9] * s[13] + t[10] * s[14]);
  d[12] = (t[2] * s[10] + t[5] * s[11] + t[1] * s[9]) - (t[4] * s[11] + t[0] * s[9] + t[3] * s[10]);
  d[13] = (t[8] * s[11] + t[0] * s[8] + t[7] * s[10]) - (t[6] * s[10] + t[9] * s[11] + t[1] * s[8]);
  d[14] = (t[6] * s[9] + t[11] * s[11] + t[3] * s[8]) - (t[10] * s[11] + t[2] * s[8] + t[7] * s[9]);
  d[15] = (t[10] * s[10] + t[4] * s[8] + t[9] * s[9]) - (t[8] * s[9] + t[11] * s[10] + t[5] * s[8]);
  det = s[0] * d[0] + s[1] * d[1] + s[2] * d[2] + s[3] * d[3];
  if (det == 0.0f) return false;
  float inv = 1.0f / det;
  for (int i = 0; i < 16; i++) d[i] *= inv;
  return true;
}

// Matrix4 * Matrix4: r(x, y) = sum_k lhs(k, y) * rhs(x, k), from 0 upwards
DM_HD void m4_mul(const float *l, const float *r, float *o) {
  for (int x = 0; x < 4; x++)
    for (int y = 0; y < 4; y++) {
      float s = 0.0f;
      for (int k = 0; k < 4; k++) s += l[k * 4 + y] * r[x * 4 + k];
      o[x * 4 + y] = s;
    }
}

// ---- ITMPose: params {tx, ty, tz, rx, ry, rz} (the twist), M = exp(params) — SetModelViewFromParams
template <class Ops>
DM_HD void pose_m_from_params(const float *prm, float *M) {
  const float one_6th = 1.0f / 6.0f, one_20th = 1.0f / 20.0f;
  const float wx = prm[3], wy = prm[4], wz = prm[5], tx = prm[0], ty = prm[1], tz = prm[2];
  const float theta_sq = wx * wx + wy * wy + wz * wz;
  float A, B, C = 0.0f, Tx, Ty, Tz;
  const float cx = wy * tz - wz * ty, cy = wz * tx - wx * tz, cz = wx * ty - wy * tx;  // cross(w, t)
  if (theta_sq < 1e-8f) {
    A = 1.0f - one_6th * theta_sq; B = 0.5f;
    Tx = tx + 0.5f * cx; Ty = ty + 0.5f * cy; Tz = tz + 0.5f * cz;
  } else {
    if (theta_sq < 1e-6f) {
      C = one_6th * (1.0f - one_20th * theta_sq);
      A = 1.0f - theta_sq * C;
      B = 0.5f - 0.25f * one_6th * theta_sq;
    } else {
      const float theta = Ops::sqrt(theta_sq);
      const float inv_theta = 1.0f / theta;
      A = sinf(theta) * inv_theta;
      B = (1.0f - cosf(theta)) * (inv_theta * inv_theta);
      C = (1.0f - A) * (inv_theta * inv_theta);
    }
    const float c2x = wy * cz - wz * cy, c2y = wz * cx - wx * cz, c2z = wx * cy - wy * cx;  // cross(w, cross(w, t))
    Tx = tx + B * cx + C * c2x; Ty = ty + B * cy + C * c2y; Tz = tz + B * cz + C * c2z;
  }
  float R[9];  // column-major m[row + 3 * col]
  const float wx2 = wx * wx, wy2 = wy * wy, wz2 = wz * wz;
  R[0 + 3 * 0] = 1.0f - B * (wy2 + wz2);
  R[1 + 3 * 1] = 1.0f - B * (wx2 + wz2);
  R[2 + 3 * 2] = 1.0f - B * (wx2 + wy2);
  float a = A * wz, b = B * (wx * wy);
  R[0 + 3 * 1] = b - a; R[1 + 3 * 0] = b + a;
  a = A * wy; b = B * (wx * wz);
  R[0 + 3 * 2] = b + a; R[2 + 3 * 0] = b - a;
  a = A * wx; b = B * (wy * wz);
  R[1 + 3 * 2] = b - a; R[2 + 3 * 1] = b + a;
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) M[c * 4 + r] = R[r + 3 * c];
  M[12] = Tx; M[13] = Ty; M[14] = Tz;
  M[3] = 0.0f; M[7] = 0.0f; M[11] = 0.0f; M[15] = 1.0f;
}

// SetParamsFromModelView: the twist of M (log map)
template <class Ops>
DM_HD void pose_params_from_m(const float *M, float *prm) {
  float R[9];
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) R[r + 3 * c] = M[c * 4 + r];
  const float Tx = M[12], Ty = M[13], Tz = M[14];
  const float cos_angle = (R[0] + R[4] + R[8] - 1.0f) * 0.5f;
  float rx = (R[2 + 3 * 1] - R[1 + 3 * 2]) * 0.5f;
  float ry = (R[0 + 3 * 2] - R[2 + 3 * 0]) * 0.5f;
  float rz = (R[1 + 3 * 0] - R[0 + 3 * 1]) * 0.5f;
  const float sin_angle_abs = Ops::sqrt(rx * rx + ry * ry + rz * rz);
  if ((double)cos_angle > 0.70710678118654752440) {  // float vs M_SQRT1_2: a double comparison, as upstream's C
    if (sin_angle_abs != 0.0f) {
      const float p = asinf<Ops>(sin_angle_abs) / sin_angle_abs;
      rx *= p; ry *= p; rz *= p;
    }
  } else if ((double)cos_angle > -0.70710678118654752440) {
    const float p = acosf<Ops>(cos_angle) / sin_angle_abs;
    rx *= p; ry *= p; rz *= p;
  } else {
    const float angle = (float)kPi - asinf<Ops>(sin_angle_abs);
    const float d0 = R[0] - cos_angle, d1 = R[4] - cos_angle, d2 = R[8] - cos_angle;
    float r2x, r2y, r2z;
    const float a0 = d0 < 0.0f ? -d0 : d0, a1 = d1 < 0.0f ? -d1 : d1, a2 = d2 < 0.0f ? -d2 : d2;
    if (a0 > a1 && a0 > a2) {
      r2x = d0; r2y = (R[1 + 3 * 0] + R[0 + 3 * 1]) / 2.0f; r2z = (R[0 + 3 * 2] + R[2 + 3 * 0]) / 2.0f;
    } else if (a1 > a2) {
      r2x = (R[1 + 3 * 0] + R[0 + 3 * 1]) / 2.0f; r2y = d1; r2z = (R[2 + 3 * 1] + R[1 + 3 * 2]) / 2.0f;
    } else {
      r2x = (R[0 + 3 * 2] + R[2 + 3 * 0]) / 2.0f; r2y = (R[2 + 3 * 1] + R[1 + 3 * 2]) / 2.0f; r2z = d2;
    }
    if (r2x * rx + r2y * ry + r2z * rz < 0.0f) { r2x *= -1.0f; r2y *= -1.0f; r2z *= -1.0f; }
    const float n = 1.0f / Ops::sqrt(r2x * r2x + r2y * r2y + r2z * r2z);
    r2x *= n; r2y *= n; r2z *= n;
    rx = angle * r2x; ry = angle * r2y; rz = angle * r2z;
  }
  // translation: the half-rotation form of TooN's SE3::ln
  const float theta = Ops::sqrt(rx * rx + ry * ry + rz * rz);
  float shtot = 0.5f;
  if (theta > 0.00001f) shtot = sinf(theta * 0.5f) / theta;
  const float half[6] = {0.0f, 0.0f, 0.0f, rx * -0.5f, ry * -0.5f, rz * -0.5f};
  float H[16];
  pose_m_from_params<Ops>(half, H);
  float ttx = H[0] * Tx + H[4] * Ty + H[8] * Tz;  // GetR() * T (Matrix3 * Vector3)
  float tty = H[1] * Tx + H[5] * Ty + H[9] * Tz;
  float ttz = H[2] * Tx + H[6] * Ty + H[10] * Tz;
  if (theta > 0.001f) {
    const float denom = rx * rx + ry * ry + rz * rz;
    const float param = (Tx * rx + Ty * ry + Tz * rz) * (1 - 2 * shtot) / denom;
    ttx -= rx * param; tty -= ry * param; ttz -= rz * param;
  } else {
    const float param = (Tx * rx + Ty * ry + Tz * rz) / 24;
    ttx -= rx * param; tty -= ry * param; ttz -= rz * param;
  }
  ttx /= 2 * shtot; tty /= 2 * shtot; ttz /= 2 * shtot;
  prm[0] = ttx; prm[1] = tty; prm[2] = ttz; prm[3] = rx; prm[4] = ry; prm[5] = rz;
}

// ITMPose::Coerce: params from M, M from params
template <class Ops>
DM_HD void pose_coerce(float *M) {
  float prm[6];
  pose_params_from_m<Ops>(M, prm);
  pose_m_from_params<Ops>(prm, M);
}

// ---- ORUtils::Cholesky (LDL^T in place) + Backsub, for n = 3 or 6; a is n x n, row-major == column-major (symmetric)
DM_HD void cholesky_solve(const float *mat, int n, const float *v, float *result) {
  float ch[36], y[6];
  for (int i = 0; i < n * n; i++) ch[i] = mat[i];
  for (int c = 0; c < n; c++) {
    float inv_diag = 1;
    for (int r = c; r < n; r++) {
      float val = ch[c + r * n];
      for (int c2 = 0; c2 < c; c2++) val -= ch[c + c2 * n] * ch[c2 + r * n];
      if (r == c) {
        ch[c + r * n] = val;
        inv_diag = 1.0f / val;
      } else {
        ch[r + c * n] = val;
        ch[c + r * n] = val * inv_diag;
      }
    }
  }
  for (int i = 0; i < n; i++) {
    float val = v[i];
    for (int j = 0; j < i; j++) val -= ch[j + i * n] * y[j];
    y[i] = val;
  }
  for (int i = 0; i < n; i++) y[i] /= ch[i + i * n];
  for (int i = n - 1; i >= 0; i--) {
    float val = y[i];
    for (int j = i + 1; j < n; j++) val -= ch[i + j * n] * result[j];
    result[i] = val;
  }
}

// ITMDepthTracker::ApplyDelta: Tinc (small-angle) * para_old.  regime: 1 rotation, 2 translation, 3 both (upstream's values)
DM_HD void apply_delta(const float *para_old, const float *delta, int regime, float *para_new) {
  float s[6];
  if (regime == 1) { s[0] = delta[0]; s[1] = delta[1]; s[2] = delta[2]; s[3] = 0.0f; s[4] = 0.0f; s[5] = 0.0f; }
  else if (regime == 2) { s[0] = 0.0f; s[1] = 0.0f; s[2] = 0.0f; s[3] = delta[0]; s[4] = delta[1]; s[5] = delta[2]; }
  else { for (int i = 0; i < 6; ++i) s[i] = delta[i]; }
  float T[16];
  T[0] = 1.0f;  T[4] = s[2];  T[8] = -s[1];  T[12] = s[3];
  T[1] = -s[2]; T[5] = 1.0f;  T[9] = s[0];   T[13] = s[4];
  T[2] = s[1];  T[6] = -s[0]; T[10] = 1.0f;  T[14] = s[5];
  T[3] = 0.0f;  T[7] = 0.0f;  T[11] = 0.0f;  T[15] = 1.0f;
  m4_mul(T, para_old, para_new);
}

}  // namespace dsr_math
