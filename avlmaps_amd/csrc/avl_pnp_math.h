// Float64 arithmetic of the image localizer (csrc/avl_pnp.hip): the sampling hash, the P3P solver, the inlier test and the pose
// update.  Plain C++ without device intrinsics, so a host compiler can build and exercise every function here as well.
// Every translation unit that includes this is compiled with -ffp-contract=off: the expressions below round as written.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define AVL_HD __host__ __device__ __forceinline__
#else
#define AVL_HD inline
#endif

namespace avl {
namespace pnp {

// ---- sampling -----------------------------------------------------------------------------------------------------------
// mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16   (uint32, wrapping)
// word(seed, h, d) = mix(mix(mix(seed ^ 0x9e3779b9) + h) + d)
// Hypothesis h draws  i0 = word(seed, h, 0) % m
//                     j  = word(seed, h, 1) % (m - 1);  i1 = j + (j >= i0)
//                     k  = word(seed, h, 2) % (m - 2);  k += (k >= min(i0, i1));  k += (k >= max(i0, i1));  i2 = k
// three distinct indices of [0, m) without rejection, a function of (seed, h, m) alone.
AVL_HD uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
AVL_HD uint32_t sample_word(uint32_t seed, uint32_t h, uint32_t d) { return mix32(mix32(mix32(seed ^ 0x9e3779b9u) + h) + d); }
AVL_HD void sample_triple(uint32_t seed, uint32_t h, uint32_t m, int32_t idx[3]) {   // m >= 3
    const uint32_t i0 = sample_word(seed, h, 0) % m;
    uint32_t i1 = sample_word(seed, h, 1) % (m - 1);
    i1 += (i1 >= i0) ? 1u : 0u;
    const uint32_t lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
    uint32_t k = sample_word(seed, h, 2) % (m - 2);
    k += (k >= lo) ? 1u : 0u;
    k += (k >= hi) ? 1u : 0u;
    idx[0] = (int32_t)i0;
    idx[1] = (int32_t)i1;
    idx[2] = (int32_t)k;
}

// ---- camera -------------------------------------------------------------------------------------------------------------
struct Camera {
    double f, cx, cy, max_err2;
};

// Camera-frame point of a 3 x 4 row-major [R|t]: every row is the left-to-right sum ((r0 X + r1 Y) + r2 Z) + t.
AVL_HD void transform(const double* P, double X, double Y, double Z, double& xc, double& yc, double& zc) {
    xc = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[3];
    yc = ((P[4] * X + P[5] * Y) + P[6] * Z) + P[7];
    zc = ((P[8] * X + P[9] * Y) + P[10] * Z) + P[11];
}

// The inlier test of the SIMPLE_PINHOLE camera: positive depth and du^2 + dv^2 <= max_err^2 with
// du = (f * (xc / zc) + cx) - u,  dv = (f * (yc / zc) + cy) - v;  a NaN or Inf in the camera point or the error is an outlier.
AVL_HD bool inlier(const double* P, const Camera& cam, double X, double Y, double Z, double u, double v) {
    double xc, yc, zc;
    transform(P, X, Y, Z, xc, yc, zc);
    if (!(zc > 0.0) || !(fabs(xc) <= 1.7976931348623157e308) || !(fabs(yc) <= 1.7976931348623157e308) || !(zc <= 1.7976931348623157e308))
        return false;
    const double du = (cam.f * (xc / zc) + cam.cx) - u;
    const double dv = (cam.f * (yc / zc) + cam.cy) - v;
    const double e = du * du + dv * dv;
    return e <= cam.max_err2;      // false for NaN
}

// ---- small polynomial roots -----------------------------------------------------------------------------------------------
// the largest real root of t^3 + A t^2 + B t + C (Numerical Recipes' trigonometric / Cardano form), two Newton steps on top
AVL_HD double cubic_largest_root(double A, double B, double C) {
    const double Q = (A * A - 3.0 * B) / 9.0;
    const double R = (2.0 * A * A * A - 9.0 * A * B + 27.0 * C) / 54.0;
    const double Q3 = Q * Q * Q;
    double t;
    if (R * R < Q3) {
        double c = R / sqrt(Q3);
        c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
        const double th = acos(c), s = -2.0 * sqrt(Q);
        const double t0 = s * cos(th / 3.0), t1 = s * cos((th + 6.283185307179586) / 3.0), t2 = s * cos((th - 6.283185307179586) / 3.0);
        t = fmax(t0, fmax(t1, t2)) - A / 3.0;
    } else {
        const double a = -(R < 0.0 ? -1.0 : 1.0) * cbrt(fabs(R) + sqrt(R * R - Q3));
        const double b = a != 0.0 ? Q / a : 0.0;
        t = (a + b) - A / 3.0;
    }
    for (int it = 0; it < 2; ++it) {
        const double fv = ((t + A) * t + B) * t + C, dv = (3.0 * t + 2.0 * A) * t + B;
        if (dv != 0.0 && fabs(fv / dv) <= 1.7976931348623157e308) t -= fv / dv;
    }
    return t;
}

// real roots of y^2 + b y + c; returns how many (0 or 2)
AVL_HD int quadratic_roots(double b, double c, double* r) {
    const double disc = b * b - 4.0 * c;
    if (!(disc >= 0.0)) return 0;
    const double s = sqrt(disc);
    const double q = -0.5 * (b + (b < 0.0 ? -s : s));
    r[0] = q;
    r[1] = q != 0.0 ? c / q : 0.0;
    return 2;
}

// real roots of c4 v^4 + c3 v^3 + c2 v^2 + c1 v + c0 by Ferrari's resolvent cubic, each polished by three Newton steps on the
// quartic itself.  Returns the number of roots written (0 .. 4); a leading coefficient that vanishes against the others gives 0.
AVL_HD int quartic_roots(const double* c, double* roots) {
    double big = 0.0;
    for (int i = 0; i < 5; ++i) big = fmax(big, fabs(c[i]));
    if (!(fabs(c[4]) > 1e-14 * big) || !(big <= 1.7976931348623157e308)) return 0;
    const double a3 = c[3] / c[4], a2 = c[2] / c[4], a1 = c[1] / c[4], a0 = c[0] / c[4];
    // y = v + a3 / 4:  y^4 + p y^2 + q y + r
    const double a3s = a3 * a3;
    const double p = a2 - 0.375 * a3s;
    const double q = a1 - 0.5 * a3 * a2 + 0.125 * a3s * a3;
    const double r = a0 - 0.25 * a3 * a1 + 0.0625 * a3s * a2 - (3.0 / 256.0) * a3s * a3s;
    double y[4];
    int n = 0;
    // m: the largest root of m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8, never negative
    const double m = cubic_largest_root(p, 0.25 * p * p - r, -0.125 * q * q);
    const double scale = fmax(1.0, fmax(fabs(p), sqrt(fabs(r))));
    if (m > 1e-14 * scale) {
        const double s = sqrt(2.0 * m), t = q / (2.0 * s);
        n += quadratic_roots(-s, 0.5 * p + m + t, y + n);
        n += quadratic_roots(s, 0.5 * p + m - t, y + n);
    } else {      // biquadratic: y^2 = z, z^2 + p z + r
        double z[2];
        if (quadratic_roots(p, r, z) == 2)
            for (int k = 0; k < 2; ++k)
                if (z[k] >= 0.0) {
                    y[n++] = sqrt(z[k]);
                    y[n++] = -sqrt(z[k]);
                }
    }
    for (int k = 0; k < n; ++k) {
        double v = y[k] - 0.25 * a3;
        for (int it = 0; it < 3; ++it) {
            const double fv = (((v + a3) * v + a2) * v + a1) * v + a0;
            const double dv = ((4.0 * v + 3.0 * a3) * v + 2.0 * a2) * v + a1;
            if (dv != 0.0 && fabs(fv / dv) <= 1.7976931348623157e308) v -= fv / dv;
        }
        roots[k] = v;
    }
    return n;
}

// ---- P3P ------------------------------------------------------------------------------------------------------------------
AVL_HD void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
AVL_HD double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// orthonormal frame of a triangle: e1 along p1 -> p2, e3 its normal, e2 = e3 x e1; false when the triangle has no area
AVL_HD bool triangle_frame(const double* p1, const double* p2, const double* p3, double E[9]) {
    double d12[3], d13[3], nrm[3];
    for (int k = 0; k < 3; ++k) {
        d12[k] = p2[k] - p1[k];
        d13[k] = p3[k] - p1[k];
    }
    cross3(d12, d13, nrm);
    const double l1 = dot3(d12, d12), l3 = dot3(nrm, nrm);
    if (!(l1 > 0.0) || !(l3 > 1e-24 * l1 * dot3(d13, d13))) return false;      // sin^2 of the angle at p1 below 1e-24: collinear
    const double i1 = 1.0 / sqrt(l1), i3 = 1.0 / sqrt(l3);
    for (int k = 0; k < 3; ++k) {
        E[k] = d12[k] * i1;
        E[6 + k] = nrm[k] * i3;
    }
    cross3(E + 6, E, E + 3);
    return true;
}

// Grunert's P3P (1841; the form of Haralick, Lee, Ottenberg, Noelle, IJCV 13(3) 1994, section 2.1).  X: three reference points
// (9 doubles), px: their query pixels (6 doubles).  With unit rays f_i, depths s_i, s2 = u s1, s3 = v s1, the law of cosines on
// the three sides a = |X2 X3|, b = |X1 X3|, c = |X1 X2| gives
//     u = ((K - 1) v^2 - 2 K cos(beta) v + 1 + K) / (2 (cos(gamma) - v cos(alpha))),   K = (a^2 - c^2) / b^2,
// and, put into  b^2 (1 + u^2 - 2 u cos(gamma)) = c^2 (1 + v^2 - 2 v cos(beta)),  a quartic in v whose coefficients are expanded
// here numerically from the two small polynomials.  s1^2 = b^2 / (1 + v^2 - 2 v cos(beta)).  Each positive (u, v) gives three
// camera points s_i f_i; [R|t] maps the reference triangle's frame onto theirs.  Returns the number of poses written to
// poses (4 x 12), 0 for repeated or collinear points and when no root is real and positive.
AVL_HD int p3p(const double* X, const double* px, const Camera& cam, double* poses) {
    double F[9];
    for (int i = 0; i < 3; ++i) {
        const double x = (px[2 * i] - cam.cx) / cam.f, y = (px[2 * i + 1] - cam.cy) / cam.f;
        const double inv = 1.0 / sqrt((x * x + y * y) + 1.0);
        F[3 * i] = x * inv;
        F[3 * i + 1] = y * inv;
        F[3 * i + 2] = inv;
    }
    double Ew[9];
    if (!triangle_frame(X, X + 3, X + 6, Ew)) return 0;
    double d[3];
    for (int k = 0; k < 3; ++k) d[k] = X[3 + k] - X[6 + k];
    const double a2 = dot3(d, d);
    for (int k = 0; k < 3; ++k) d[k] = X[k] - X[6 + k];
    const double b2 = dot3(d, d);
    for (int k = 0; k < 3; ++k) d[k] = X[k] - X[3 + k];
    const double c2 = dot3(d, d);
    if (!(a2 > 0.0) || !(b2 > 0.0) || !(c2 > 0.0)) return 0;
    const double ca = dot3(F + 3, F + 6), cb = dot3(F, F + 6), cg = dot3(F, F + 3);
    const double K = (a2 - c2) / b2, cr = c2 / b2;
    // N(v) = n2 v^2 + n1 v + n0,  D(v) = d1 v + d0,  G(v) = v^2 - 2 cb v + 1
    const double n2 = K - 1.0, n1 = -2.0 * K * cb, n0 = 1.0 + K, d1 = -2.0 * ca, d0 = 2.0 * cg;
    const double DD[3] = {d0 * d0, 2.0 * d0 * d1, d1 * d1};                                      // D^2
    const double NN[5] = {n0 * n0, 2.0 * n0 * n1, 2.0 * n0 * n2 + n1 * n1, 2.0 * n1 * n2, n2 * n2};   // N^2
    const double ND[4] = {n0 * d0, n0 * d1 + n1 * d0, n1 * d1 + n2 * d0, n2 * d1};               // N D
    const double G[3] = {1.0, -2.0 * cb, 1.0};
    double GD[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                                                    // G D^2
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) GD[i + j] += G[i] * DD[j];
    // (D^2 + N^2 - 2 cg N D) - (c^2 / b^2) G D^2
    double q[5];
    for (int i = 0; i < 5; ++i) {
        const double dd = i < 3 ? DD[i] : 0.0, nd = i < 4 ? ND[i] : 0.0;
        q[i] = ((dd + NN[i]) - 2.0 * cg * nd) - cr * GD[i];
    }
    double roots[4];
    const int nr = quartic_roots(q, roots);
    int ns = 0;
    for (int k = 0; k < nr; ++k) {
        const double v = roots[k];
        if (!(v > 0.0)) continue;
        const double den = d1 * v + d0;
        const double g = (v - 2.0 * cb) * v + 1.0;
        if (!(fabs(den) > 1e-12) || !(g > 0.0)) continue;
        const double u = ((n2 * v + n1) * v + n0) / den;
        if (!(u > 0.0)) continue;
        const double s1 = sqrt(b2 / g), s2 = u * s1, s3 = v * s1;
        double C[9], Ec[9];
        for (int j = 0; j < 3; ++j) {
            C[j] = s1 * F[j];
            C[3 + j] = s2 * F[3 + j];
            C[6 + j] = s3 * F[6 + j];
        }
        if (!triangle_frame(C, C + 3, C + 6, Ec)) continue;
        double* P = poses + 12 * ns;
        bool ok = true;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) P[4 * i + j] = (Ec[i] * Ew[j] + Ec[3 + i] * Ew[3 + j]) + Ec[6 + i] * Ew[6 + j];   // Ec^T-columns x Ew rows
            P[4 * i + 3] = C[i] - ((P[4 * i] * X[0] + P[4 * i + 1] * X[1]) + P[4 * i + 2] * X[2]);
            for (int j = 0; j < 4; ++j) ok = ok && (fabs(P[4 * i + j]) <= 1.7976931348623157e308);
        }
        if (ok) ++ns;
    }
    return ns;
}

// ---- refinement -----------------------------------------------------------------------------------------------------------
constexpr int kNormal = 28;      // 21 entries of the upper triangle of J^T J, row by row, then 6 of J^T r, then the cost

// One correspondence's residual and its share of the normal equations for the update  R <- exp([w]x) R, t <- t + dt
// (parameters w0 w1 w2 dt0 dt1 dt2).  With Y = R X and (x, y, z) = Y + t:  d(x y z)/dw = -[Y]x,  d(x y z)/dt = I,
// du = f (dx / z - x dz / z^2),  dv = f (dy / z - y dz / z^2).  false (nothing added) when the point is not in front.
AVL_HD bool normal_terms(const double* P, const Camera& cam, double X, double Y, double Z, double u, double v, double* acc) {
    const double Yx = (P[0] * X + P[1] * Y) + P[2] * Z, Yy = (P[4] * X + P[5] * Y) + P[6] * Z, Yz = (P[8] * X + P[9] * Y) + P[10] * Z;
    const double x = Yx + P[3], y = Yy + P[7], z = Yz + P[11];
    if (!(z > 0.0) || !(z <= 1.7976931348623157e308)) return false;
    const double iz = 1.0 / z;
    const double ru = (cam.f * (x / z) + cam.cx) - u, rv = (cam.f * (y / z) + cam.cy) - v;
    const double gx = cam.f * iz, gux = -cam.f * x * iz * iz, gvy = -cam.f * y * iz * iz;      // du/dx = dv/dy, du/dz, dv/dz
    // d(x y z)/dw columns: w0 -> (0, -Yz, Yy)... as rows of -[Y]x: dx = (0, Yz, -Yy), dy = (-Yz, 0, Yx), dz = (Yy, -Yx, 0)
    const double Ju[6] = {gux * Yy, gx * Yz - gux * Yx, -gx * Yy, gx, 0.0, gux};
    const double Jv[6] = {-gx * Yz + gvy * Yy, -gvy * Yx, gx * Yx, 0.0, gx, gvy};
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) acc[k++] += Ju[i] * Ju[j] + Jv[i] * Jv[j];
    for (int i = 0; i < 6; ++i) acc[21 + i] += Ju[i] * ru + Jv[i] * rv;
    acc[27] += ru * ru + rv * rv;
    return true;
}

// solves (A + lambda diag(A)) d = -g for the 6 x 6 system kept in `acc` (Gaussian elimination, partial pivoting); false when singular
AVL_HD bool solve_step(const double* acc, double lambda, double* d) {
    double A[6][7];
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) {
            A[i][j] = acc[k];
            A[j][i] = acc[k];
            ++k;
        }
    for (int i = 0; i < 6; ++i) {
        A[i][i] += lambda * A[i][i];
        A[i][6] = -acc[21 + i];
    }
    for (int c = 0; c < 6; ++c) {
        int piv = c;
        for (int r = c + 1; r < 6; ++r)
            if (fabs(A[r][c]) > fabs(A[piv][c])) piv = r;
        if (!(fabs(A[piv][c]) > 0.0) || !(fabs(A[piv][c]) <= 1.7976931348623157e308)) return false;
        if (piv != c)
            for (int j = 0; j < 7; ++j) {
                const double t = A[c][j];
                A[c][j] = A[piv][j];
                A[piv][j] = t;
            }
        for (int r = c + 1; r < 6; ++r) {
            const double m = A[r][c] / A[c][c];
            for (int j = c; j < 7; ++j) A[r][j] -= m * A[c][j];
        }
    }
    for (int i = 5; i >= 0; --i) {
        double s = A[i][6];
        for (int j = i + 1; j < 6; ++j) s -= A[i][j] * d[j];
        d[i] = s / A[i][i];
    }
    for (int i = 0; i < 6; ++i)
        if (!(fabs(d[i]) <= 1.7976931348623157e308)) return false;
    return true;
}

// Pout = [exp([w]x) R | t + dt]  (Rodrigues' formula), w = d[0..2], dt = d[3..5]
AVL_HD void apply_step(const double* P, const double* d, double* Pout) {
    const double th2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], th = sqrt(th2);
    double a, b;      // exp = I + a [w]x + b [w]x^2
    if (th < 1e-8) {
        a = 1.0 - th2 / 6.0;
        b = 0.5 - th2 / 24.0;
    } else {
        a = sin(th) / th;
        b = (1.0 - cos(th)) / th2;
    }
    const double wx = d[0], wy = d[1], wz = d[2];
    const double E[9] = {1.0 - b * (wy * wy + wz * wz), -a * wz + b * wx * wy,         a * wy + b * wx * wz,
                         a * wz + b * wx * wy,          1.0 - b * (wx * wx + wz * wz), -a * wx + b * wy * wz,
                         -a * wy + b * wx * wz,         a * wx + b * wy * wz,          1.0 - b * (wx * wx + wy * wy)};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) Pout[4 * i + j] = (E[3 * i] * P[j] + E[3 * i + 1] * P[4 + j]) + E[3 * i + 2] * P[8 + j];
        Pout[4 * i + 3] = P[4 * i + 3] + d[3 + i];
    }
}

}  // namespace pnp
}  // namespace avl
