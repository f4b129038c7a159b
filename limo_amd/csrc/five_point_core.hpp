// five_point_core.hpp — the five-point motion prior, one statement for the host and for gfx950 lanes.
//
// Replaces what the reference gets from OpenCV at
//   keyframe_bundle_adjustment_ros_tool/src/commons/general_helpers.hpp:103-140  calcMotion5Point: cv::findEssentialMat(points1,
//                                                                                points0, focal, pp, RANSAC, probability, 2.0)
//                                                                                + cv::recoverPose
//   :209-231                                                                     getMotionUnscaled (its caller; stays with the driver)
// and restates limo_amd/kba/five_point.hpp (the host estimator, which stays the checker of this file) without std::vector,
// std::complex, std::array or std::sort: the same floating-point operations in the same order, on plain arrays, so that a lane of
// five_point.hip and the host give the same bits.  BIT-EXACT CONTRACT: compiled with floating-point contraction off on both sides
// (#pragma clang fp contract(off) + -ffp-contract=off in the build, as for landmark_init.hip); every operation is one of
// + - * / sqrt fabs or a comparison - all correctly rounded on gfx950 - and no sum is reassociated.  pow / log (the adaptive
// sample count) are host statements: fp5::Scan below.
//
// A sample's working set (the 10 x 20 elimination matrix, the action matrix, its shifted copy ...) is kWs doubles, handed in by
// the caller: LDS on the device (it fits no register file and must not live in scratch), the stack on the host.
#pragma once
#include <math.h>
#include <stdint.h>

#include "kba_math.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace kba {
namespace fp5 {

// ---- working set of one minimal sample, in doubles.  Regions are reused once their content is dead:
//   kE  36   null-space basis: entry e of E(x, y, z) = x X + y Y + z Z + W as [X_e Y_e Z_e W_e]
//   kA  100  polynomial temporaries while the cubics are built; then the action matrix
//   kM  200  sort order of the null space; the ten cubics / the elimination matrix; then the shifted copy (100), wr, wi, v, u, found
//   kX  162  Q^T Q (81) and its eigenvectors (81); then E E^T / L (90) and the 2 x 2 minors (30), trace (10)
constexpr int kE = 0, kA = 36, kM = 136, kX = 336, kWs = 498;
constexpr int kMaxModels = 10;

KBA_HD bool finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // (false for NaN)

// ---- monomial tables of five_point.hpp:41-81, as literals.  kT11[p][q]: index of (degree-1 monomial p) * (degree-1 monomial q) in
//      [x2 xy xz y2 yz z2 x y z 1]; kT21[p][q]: index of (degree-2 monomial p) * (degree-1 monomial q) in the degree-3 list
struct Tables {
    int t11[4][4];
    int t21[10][4];
};
constexpr Tables make_tables() {
    const int m1[4][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 0, 0}};
    const int m2[10][3] = {{2, 0, 0}, {1, 1, 0}, {1, 0, 1}, {0, 2, 0}, {0, 1, 1}, {0, 0, 2}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 0, 0}};
    const int m3[20][3] = {{3, 0, 0}, {2, 1, 0}, {2, 0, 1}, {1, 2, 0}, {1, 1, 1}, {1, 0, 2}, {0, 3, 0}, {0, 2, 1}, {0, 1, 2}, {0, 0, 3},
                           {2, 0, 0}, {1, 1, 0}, {1, 0, 1}, {0, 2, 0}, {0, 1, 1}, {0, 0, 2}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 0, 0}};
    Tables t{};
    for (int p = 0; p < 4; ++p)
        for (int q = 0; q < 4; ++q) {
            t.t11[p][q] = -1;
            for (int k = 0; k < 10; ++k)
                if (m2[k][0] == m1[p][0] + m1[q][0] && m2[k][1] == m1[p][1] + m1[q][1] && m2[k][2] == m1[p][2] + m1[q][2]) {
                    t.t11[p][q] = k;
                    break;
                }
        }
    for (int p = 0; p < 10; ++p)
        for (int q = 0; q < 4; ++q) {
            t.t21[p][q] = -1;
            for (int k = 0; k < 20; ++k)
                if (m3[k][0] == m2[p][0] + m1[q][0] && m3[k][1] == m2[p][1] + m1[q][1] && m3[k][2] == m2[p][2] + m1[q][2]) {
                    t.t21[p][q] = k;
                    break;
                }
        }
    return t;
}

KBA_HD void mul11(const double* a, const double* b, double* c) {  // five_point.hpp:58-69
    constexpr Tables T = make_tables();
    for (int k = 0; k < 10; ++k) c[k] = 0.;
    for (int p = 0; p < 4; ++p)
        for (int q = 0; q < 4; ++q) c[T.t11[p][q]] += a[p] * b[q];
}
KBA_HD void mul21(const double* a, const double* b, double* c) {  // :70-81
    constexpr Tables T = make_tables();
    for (int k = 0; k < 20; ++k) c[k] = 0.;
    for (int p = 0; p < 10; ++p)
        for (int q = 0; q < 4; ++q) c[T.t21[p][q]] += a[p] * b[q];
}
// c = a + sb * b (:82-87); c may be a
KBA_HD void add(int n, const double* a, const double* b, double sb, double* c) {
    for (int q = 0; q < n; ++q) c[q] = a[q] + sb * b[q];
}

// eigenvectors of a symmetric N x N matrix by cyclic Jacobi rotations (:89-123); a is destroyed, its diagonal holds the eigenvalues.
// `order` (N doubles holding small integers) receives the ascending order of the diagonal, as std::sort leaves it for N <= 16: a
// straight insertion sort (:124-126)
template <int N>
KBA_HD void symmetric_eigen(double* a, double* V, double* order) {
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) V[i * N + j] = i == j ? 1. : 0.;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.;
        for (int i = 0; i < N; ++i)
            for (int j = i + 1; j < N; ++j) off += a[i * N + j] * a[i * N + j];
        double diag = 0.;
        for (int i = 0; i < N; ++i) diag += a[i * N + i] * a[i * N + i];
        if (off <= 1e-32 * diag || off < 1e-300) break;
        for (int p = 0; p < N; ++p)
            for (int q = p + 1; q < N; ++q) {
                if (fabs(a[p * N + q]) < 1e-300) continue;
                const double theta = (a[q * N + q] - a[p * N + p]) / (2. * a[p * N + q]);
                const double t = (theta >= 0. ? 1. : -1.) / (fabs(theta) + sqrt(theta * theta + 1.));
                const double c = 1. / sqrt(t * t + 1.), s = t * c;
                for (int k = 0; k < N; ++k) {  // A <- A J
                    const double akp = a[k * N + p], akq = a[k * N + q];
                    a[k * N + p] = c * akp - s * akq;
                    a[k * N + q] = s * akp + c * akq;
                }
                for (int k = 0; k < N; ++k) {  // A <- J^T A
                    const double apk = a[p * N + k], aqk = a[q * N + k];
                    a[p * N + k] = c * apk - s * aqk;
                    a[q * N + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < N; ++k) {
                    const double vkp = V[k * N + p], vkq = V[k * N + q];
                    V[k * N + p] = c * vkp - s * vkq;
                    V[k * N + q] = s * vkp + c * vkq;
                }
            }
    }
    for (int i = 0; i < N; ++i) order[i] = (double)i;
    for (int i = 1; i < N; ++i) {
        const int val = (int)order[i];
        const double key = a[val * N + val];
        const int first = (int)order[0];
        if (key < a[first * N + first]) {
            for (int j = i; j > 0; --j) order[j] = order[j - 1];
            order[0] = (double)val;
        } else {
            int j = i;
            while (true) {
                const int prev = (int)order[j - 1];
                if (!(key < a[prev * N + prev])) break;
                order[j] = order[j - 1];
                --j;
            }
            order[j] = (double)val;
        }
    }
}

// solve a x = b in place by Gaussian elimination with partial pivoting, 10 x 10 (:136-159); a is destroyed
KBA_HD bool solve10(double* a, double* b) {
    for (int c = 0; c < 10; ++c) {
        int piv = c;
        for (int r = c + 1; r < 10; ++r)
            if (fabs(a[r * 10 + c]) > fabs(a[piv * 10 + c])) piv = r;
        if (fabs(a[piv * 10 + c]) < 1e-300) return false;
        if (piv != c) {
            for (int k = 0; k < 10; ++k) {
                const double x = a[piv * 10 + k];
                a[piv * 10 + k] = a[c * 10 + k];
                a[c * 10 + k] = x;
            }
            const double x = b[piv];
            b[piv] = b[c];
            b[c] = x;
        }
        for (int r = c + 1; r < 10; ++r) {
            const double f = a[r * 10 + c] / a[c * 10 + c];
            if (f == 0.) continue;
            for (int k = c; k < 10; ++k) a[r * 10 + k] -= f * a[c * 10 + k];
            b[r] -= f * b[c];
        }
    }
    for (int r = 9; r >= 0; --r) {
        double s = b[r];
        for (int k = r + 1; k < 10; ++k) s -= a[r * 10 + k] * b[k];
        b[r] = s / a[r * 10 + r];
    }
    return true;
}

// eigenvalues of a real 10 x 10 matrix: elmhes + hqr (:164-313); a is destroyed
KBA_HD bool eigenvalues10(double* a, double* wr, double* wi) {
    constexpr int n = 10;
#define FP5_A(i, j) a[(i) * n + (j)]
    for (int m = 1; m < n - 1; ++m) {
        double x = 0.;
        int piv = m;
        for (int j = m; j < n; ++j)
            if (fabs(FP5_A(j, m - 1)) > fabs(x)) {
                x = FP5_A(j, m - 1);
                piv = j;
            }
        if (piv != m) {
            for (int j = m - 1; j < n; ++j) {
                const double s = FP5_A(piv, j);
                FP5_A(piv, j) = FP5_A(m, j);
                FP5_A(m, j) = s;
            }
            for (int j = 0; j < n; ++j) {
                const double s = FP5_A(j, piv);
                FP5_A(j, piv) = FP5_A(j, m);
                FP5_A(j, m) = s;
            }
        }
        if (x != 0.)
            for (int i = m + 1; i < n; ++i) {
                double y = FP5_A(i, m - 1);
                if (y == 0.) continue;
                y /= x;
                FP5_A(i, m - 1) = y;
                for (int j = m; j < n; ++j) FP5_A(i, j) -= y * FP5_A(m, j);
                for (int j = 0; j < n; ++j) FP5_A(j, m) += y * FP5_A(j, i);
            }
    }
    for (int i = 2; i < n; ++i)
        for (int j = 0; j < i - 1; ++j) FP5_A(i, j) = 0.;
    double anorm = 0.;
    for (int i = 0; i < n; ++i)
        for (int j = (i - 1 > 0 ? i - 1 : 0); j < n; ++j) anorm += fabs(FP5_A(i, j));
    int nn = n - 1;
    double t = 0.;
    while (nn >= 0) {
        int its = 0, l;
        do {
            for (l = nn; l >= 1; --l) {
                double s = fabs(FP5_A(l - 1, l - 1)) + fabs(FP5_A(l, l));
                if (s == 0.) s = anorm;
                if (fabs(FP5_A(l, l - 1)) + s == s) {
                    FP5_A(l, l - 1) = 0.;
                    break;
                }
            }
            double x = FP5_A(nn, nn);
            if (l == nn) {
                wr[nn] = x + t;
                wi[nn] = 0.;
                --nn;
            } else {
                double y = FP5_A(nn - 1, nn - 1), w = FP5_A(nn, nn - 1) * FP5_A(nn - 1, nn);
                if (l == nn - 1) {
                    const double p = 0.5 * (y - x), q = p * p + w;
                    double z = sqrt(fabs(q));
                    x += t;
                    if (q >= 0.) {
                        z = p + (p >= 0. ? fabs(z) : -fabs(z));
                        wr[nn - 1] = wr[nn] = x + z;
                        if (z != 0.) wr[nn] = x - w / z;
                        wi[nn - 1] = wi[nn] = 0.;
                    } else {
                        wr[nn - 1] = wr[nn] = x + p;
                        wi[nn] = z;
                        wi[nn - 1] = -z;
                    }
                    nn -= 2;
                } else {
                    if (its == 60) return false;
                    if (its == 10 || its == 20 || its == 30 || its == 40 || its == 50) {
                        t += x;
                        for (int i = 0; i <= nn; ++i) FP5_A(i, i) -= x;
                        const double s = fabs(FP5_A(nn, nn - 1)) + fabs(FP5_A(nn - 1, nn - 2));
                        y = x = 0.75 * s;
                        w = -0.4375 * s * s;
                    }
                    ++its;
                    int m;
                    double p = 0., q = 0., r = 0., z;
                    for (m = nn - 2; m >= l; --m) {
                        z = FP5_A(m, m);
                        r = x - z;
                        double s = y - z;
                        p = (r * s - w) / FP5_A(m + 1, m) + FP5_A(m, m + 1);
                        q = FP5_A(m + 1, m + 1) - z - r - s;
                        r = FP5_A(m + 2, m + 1);
                        s = fabs(p) + fabs(q) + fabs(r);
                        p /= s;
                        q /= s;
                        r /= s;
                        if (m == l) break;
                        const double u = fabs(FP5_A(m, m - 1)) * (fabs(q) + fabs(r));
                        const double v = fabs(p) * (fabs(FP5_A(m - 1, m - 1)) + fabs(z) + fabs(FP5_A(m + 1, m + 1)));
                        if (u + v == v) break;
                    }
                    for (int i = m + 2; i <= nn; ++i) {
                        FP5_A(i, i - 2) = 0.;
                        if (i != m + 2) FP5_A(i, i - 3) = 0.;
                    }
                    for (int k = m; k <= nn - 1; ++k) {
                        if (k != m) {
                            p = FP5_A(k, k - 1);
                            q = FP5_A(k + 1, k - 1);
                            r = k != nn - 1 ? FP5_A(k + 2, k - 1) : 0.;
                            x = fabs(p) + fabs(q) + fabs(r);
                            if (x != 0.) {
                                p /= x;
                                q /= x;
                                r /= x;
                            }
                        }
                        const double nrm = sqrt(p * p + q * q + r * r);
                        const double s = p >= 0. ? nrm : -nrm;
                        if (s != 0.) {
                            if (k == m) {
                                if (l != m) FP5_A(k, k - 1) = -FP5_A(k, k - 1);
                            } else {
                                FP5_A(k, k - 1) = -s * x;
                            }
                            p += s;
                            x = p / s;
                            y = q / s;
                            z = r / s;
                            q /= p;
                            r /= p;
                            for (int j = k; j <= nn; ++j) {
                                p = FP5_A(k, j) + q * FP5_A(k + 1, j);
                                if (k != nn - 1) {
                                    p += r * FP5_A(k + 2, j);
                                    FP5_A(k + 2, j) -= p * z;
                                }
                                FP5_A(k + 1, j) -= p * y;
                                FP5_A(k, j) -= p * x;
                            }
                            const int mmin = nn < k + 3 ? nn : k + 3;
                            for (int i = l; i <= mmin; ++i) {
                                p = x * FP5_A(i, k) + y * FP5_A(i, k + 1);
                                if (k != nn - 1) {
                                    p += z * FP5_A(i, k + 2);
                                    FP5_A(i, k + 2) -= p * r;
                                }
                                FP5_A(i, k + 1) -= p * q;
                                FP5_A(i, k) -= p;
                            }
                        }
                    }
                }
            }
        } while (l < nn - 1);
    }
#undef FP5_A
    return true;
}

// null-space basis (ws + kE) and action matrix (ws + kA) of five correspondences in normalised coordinates (:330-388);
// false for a degenerate sample
KBA_HD bool action_matrix(const double* sa /* [5][2] */, const double* sb, double* ws) {
    double* E = ws + kE;
    {   // null space of the 5 x 9 constraint matrix: the four eigenvectors of Q^T Q with the smallest eigenvalues
        double* QtQ = ws + kX;
        double* V = ws + kX + 81;
        double* order = ws + kM;
        double* q = ws + kM + 16;
        for (int i = 0; i < 81; ++i) QtQ[i] = 0.;
        for (int p = 0; p < 5; ++p) {
            const double a0 = sa[2 * p], a1 = sa[2 * p + 1], b0 = sb[2 * p], b1 = sb[2 * p + 1];
            q[0] = b0 * a0;
            q[1] = b0 * a1;
            q[2] = b0;
            q[3] = b1 * a0;
            q[4] = b1 * a1;
            q[5] = b1;
            q[6] = a0;
            q[7] = a1;
            q[8] = 1.;
            for (int i = 0; i < 9; ++i)
                for (int j = 0; j < 9; ++j) QtQ[i * 9 + j] += q[i] * q[j];
        }
        symmetric_eigen<9>(QtQ, V, order);
        for (int e = 0; e < 9; ++e)
            for (int c = 0; c < 4; ++c) E[e * 4 + c] = V[e * 9 + (int)order[c]];
    }
    double* M = ws + kM;  // the ten cubics, row r at M + 20 r
    {
        double* EEt = ws + kX;        // [9][10], becomes L
        double* m0 = ws + kX + 90;    // the three 2 x 2 minors of rows 1, 2
        double* m1 = ws + kX + 100;
        double* m2 = ws + kX + 110;
        double* tr = ws + kX + 120;
        double* t2 = ws + kA;         // degree-2 temporary
        double* t3 = ws + kA + 10;    // degree-3 temporary
#define FP5_E(e) (E + 4 * (e))
        mul11(FP5_E(4), FP5_E(8), m0);
        mul11(FP5_E(5), FP5_E(7), t2);
        add(10, m0, t2, -1., m0);
        mul11(FP5_E(3), FP5_E(8), m1);
        mul11(FP5_E(5), FP5_E(6), t2);
        add(10, m1, t2, -1., m1);
        mul11(FP5_E(3), FP5_E(7), m2);
        mul11(FP5_E(4), FP5_E(6), t2);
        add(10, m2, t2, -1., m2);
        mul21(m0, FP5_E(0), M);  // det E
        mul21(m1, FP5_E(1), t3);
        add(20, M, t3, -1., M);
        mul21(m2, FP5_E(2), t3);
        add(20, M, t3, 1., M);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double* d = EEt + 10 * (3 * i + j);
                mul11(FP5_E(3 * i), FP5_E(3 * j), d);
                mul11(FP5_E(3 * i + 1), FP5_E(3 * j + 1), t2);
                add(10, d, t2, 1., d);
                mul11(FP5_E(3 * i + 2), FP5_E(3 * j + 2), t2);
                add(10, d, t2, 1., d);
            }
        add(10, EEt, EEt + 40, 1., tr);
        add(10, tr, EEt + 80, 1., tr);
        for (int d = 0; d < 9; d += 4) add(10, EEt + 10 * d, tr, -0.5, EEt + 10 * d);  // L = E E^T - 1/2 tr(E E^T) I
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double* d = M + 20 * (1 + 3 * i + j);
                mul21(EEt + 10 * (3 * i), FP5_E(j), d);
                mul21(EEt + 10 * (3 * i + 1), FP5_E(3 + j), t3);
                add(20, d, t3, 1., d);
                mul21(EEt + 10 * (3 * i + 2), FP5_E(6 + j), t3);
                add(20, d, t3, 1., d);
            }
#undef FP5_E
    }
    // Gauss-Jordan on the ten degree-3 columns: [I | B]
    for (int c = 0; c < 10; ++c) {
        int piv = c;
        for (int r = c + 1; r < 10; ++r)
            if (fabs(M[r * 20 + c]) > fabs(M[piv * 20 + c])) piv = r;
        if (fabs(M[piv * 20 + c]) < 1e-14) return false;  // degenerate sample
        for (int k = 0; k < 20; ++k) {
            const double x = M[piv * 20 + k];
            M[piv * 20 + k] = M[c * 20 + k];
            M[c * 20 + k] = x;
        }
        const double inv = 1. / M[c * 20 + c];
        for (int k = 0; k < 20; ++k) M[c * 20 + k] *= inv;
        for (int r = 0; r < 10; ++r) {
            if (r == c) continue;
            const double f = M[r * 20 + c];
            if (f == 0.) continue;
            for (int k = 0; k < 20; ++k) M[r * 20 + k] -= f * M[c * 20 + k];
        }
    }
    double* A = ws + kA;
    for (int i = 0; i < 100; ++i) A[i] = 0.;
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 10; ++c) A[r * 10 + c] = -M[r * 20 + 10 + c];
    A[6 * 10 + 0] = 1.;
    A[7 * 10 + 1] = 1.;
    A[8 * 10 + 2] = 1.;
    A[9 * 10 + 6] = 1.;
    return true;
}

// essential matrices consistent with five correspondences (:390-463): up to ten, |E|_F = 1, nine doubles each at out + 9 k, in the
// order the host's vector holds them.  Returns their number.
KBA_HD int essential_from_five(const double* sa, const double* sb, double* ws, double* out) {
    if (!action_matrix(sa, sb, ws)) return 0;
    const double* E = ws + kE;
    const double* A = ws + kA;
    double* S = ws + kM;
    double* wr = ws + kM + 100;
    double* wi = ws + kM + 110;
    double* v = ws + kM + 120;
    double* u = ws + kM + 130;
    double* found = ws + kM + 140;
    for (int i = 0; i < 100; ++i) S[i] = A[i];
    if (!eigenvalues10(S, wr, wi)) return 0;
    int n_out = 0, n_found = 0;
    double a_scale = 0.;
    for (int i = 0; i < 100; ++i) {
        const double f = fabs(A[i]);
        a_scale = a_scale < f ? f : a_scale;
    }
    for (int root = 0; root < 10; ++root) {
        if (fabs(wi[root]) > 1e-4 * (1. + fabs(wr[root]))) continue;
        double lambda = wr[root];
        for (int i = 0; i < 10; ++i) v[i] = 1. / (1. + i);
        bool ok = true;
        for (int it = 0; it < 8 && ok; ++it) {
            for (int i = 0; i < 100; ++i) S[i] = A[i];
            const double shift = lambda + 1e-9 * (1. + fabs(lambda));
            for (int i = 0; i < 10; ++i) S[i * 10 + i] -= shift;
            for (int i = 0; i < 10; ++i) u[i] = v[i];
            ok = solve10(S, u);
            if (!ok) break;
            double uu = 0., uv = 0.;
            for (int i = 0; i < 10; ++i) {
                uu += u[i] * u[i];
                uv += u[i] * v[i];
            }
            if (!(uu > 0.) || !finite(uu) || uv == 0.) {
                ok = false;
                break;
            }
            double vv = 0.;
            for (int i = 0; i < 10; ++i) vv += v[i] * v[i];
            const double lambda_new = shift + vv / uv;
            const bool settled = it >= 1 && fabs(lambda_new - lambda) <= 1e-13 * (1. + fabs(lambda_new));
            lambda = lambda_new;
            const double n = sqrt(uu);
            for (int i = 0; i < 10; ++i) v[i] = u[i] / n;
            if (settled) break;
        }
        if (!ok || !finite(lambda)) continue;
        double res = 0.;
        for (int i = 0; i < 10; ++i) {
            double sacc = -lambda * v[i];
            for (int q = 0; q < 10; ++q) sacc += A[i * 10 + q] * v[q];
            res += sacc * sacc;
        }
        if (sqrt(res) > 1e-7 * (a_scale + fabs(lambda))) continue;
        bool seen = false;
        for (int k = 0; k < n_found; ++k) seen = seen || fabs(found[k] - lambda) <= 1e-7 * (1. + fabs(lambda));
        if (seen || fabs(v[9]) < 1e-12) continue;
        found[n_found++] = lambda;
        const double x = v[6] / v[9], y = v[7] / v[9], zc = v[8] / v[9];
        double* Em = out + 9 * n_out;
        double n = 0.;
        for (int e = 0; e < 9; ++e) {
            const double em = x * E[e * 4 + 0] + y * E[e * 4 + 1] + zc * E[e * 4 + 2] + E[e * 4 + 3];
            Em[e] = em;
            n += em * em;
        }
        n = sqrt(n);
        if (!(n > 0.) || !finite(n)) continue;
        for (int e = 0; e < 9; ++e) Em[e] /= n;
        ++n_out;
    }
    return n_out;
}

// squared Sampson distance of a correspondence (normalised coordinates) to b^T E a = 0 (:466-472)
KBA_HD double sampson2(const double* E, double a0, double a1, double b0, double b1) {
    const double Ea0 = E[0] * a0 + E[1] * a1 + E[2], Ea1 = E[3] * a0 + E[4] * a1 + E[5], Ea2 = E[6] * a0 + E[7] * a1 + E[8];
    const double Etb0 = E[0] * b0 + E[3] * b1 + E[6], Etb1 = E[1] * b0 + E[4] * b1 + E[7];
    const double r = b0 * Ea0 + b1 * Ea1 + Ea2;
    const double d = Ea0 * Ea0 + Ea1 * Ea1 + Etb0 * Etb0 + Etb1 * Etb1;
    return d > 0. ? r * r / d : 1e300;
}

// the four decompositions of E (:486-529): candidate c has rotation cand + 12 c (row-major) and translation cand + 12 c + 9.
// ws: 24 doubles of scratch (E^T E, its eigenvectors, the sort order)
KBA_HD void pose_candidates(const double* E, double* ws, double* cand /* [4][12] */) {
    double* EtE = ws;
    double* Vc = ws + 9;
    double* order = ws + 18;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) EtE[3 * i + j] = E[i] * E[j] + E[3 + i] * E[3 + j] + E[6 + i] * E[6 + j];
    symmetric_eigen<3>(EtE, Vc, order);  // ascending: column order[0] = null direction of E
    double V[3][3], U[3][3];
    const int o0 = (int)order[0], o1 = (int)order[1], o2 = (int)order[2];
    for (int r = 0; r < 3; ++r) {
        V[r][0] = Vc[r * 3 + o2];
        V[r][1] = Vc[r * 3 + o1];
        V[r][2] = Vc[r * 3 + o0];
    }
    for (int c = 0; c < 2; ++c) {
        const double u0 = E[0] * V[0][c] + E[1] * V[1][c] + E[2] * V[2][c], u1 = E[3] * V[0][c] + E[4] * V[1][c] + E[5] * V[2][c],
                     u2 = E[6] * V[0][c] + E[7] * V[1][c] + E[8] * V[2][c];
        const double n = sqrt(u0 * u0 + u1 * u1 + u2 * u2);
        U[0][c] = n > 0. ? u0 / n : (0 == c ? 1. : 0.);
        U[1][c] = n > 0. ? u1 / n : (1 == c ? 1. : 0.);
        U[2][c] = n > 0. ? u2 / n : 0.;
    }
    U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
    U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
    U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
    {
        const double d = V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0]) +
                         V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]);
        if (d < 0.)
            for (int r = 0; r < 3; ++r) V[r][2] = -V[r][2];
    }
    for (int c4 = 0; c4 < 4; ++c4) {
        // W = [0 -1 0; 1 0 0; 0 0 1] for even candidates, its transpose for odd ones
        const double w01 = (c4 & 1) ? 1. : -1., w10 = (c4 & 1) ? -1. : 1.;
        const double Wc[9] = {0., w01, 0., w10, 0., 0., 0., 0., 1.};
        double UW[9], R[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) UW[3 * i + j] = U[i][0] * Wc[j] + U[i][1] * Wc[3 + j] + U[i][2] * Wc[6 + j];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[3 * i + j] = UW[3 * i] * V[j][0] + UW[3 * i + 1] * V[j][1] + UW[3 * i + 2] * V[j][2];
        const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        if (det < 0.)
            for (int i = 0; i < 9; ++i) R[i] = -R[i];
        const double sgn = (c4 & 2) ? -1. : 1.;
        for (int i = 0; i < 9; ++i) cand[12 * c4 + i] = R[i];
        for (int i = 0; i < 3; ++i) cand[12 * c4 + 9 + i] = sgn * U[i][2];
    }
}

// one inlier in front of both cameras of candidate (R, t) (:534-544)
KBA_HD bool in_front(const double* R, const double* t, double a0, double a1, double b0, double b1) {
    const double xa[3] = {a0, a1, 1.}, xb[3] = {b0, b1, 1.};
    const double ra[3] = {R[0] * xa[0] + R[1] * xa[1] + R[2] * xa[2], R[3] * xa[0] + R[4] * xa[1] + R[5] * xa[2],
                          R[6] * xa[0] + R[7] * xa[1] + R[8] * xa[2]};
    const double a11 = ra[0] * ra[0] + ra[1] * ra[1] + ra[2] * ra[2], a12 = -(ra[0] * xb[0] + ra[1] * xb[1] + ra[2] * xb[2]),
                 a22 = xb[0] * xb[0] + xb[1] * xb[1] + xb[2] * xb[2];
    const double b1_ = -(ra[0] * t[0] + ra[1] * t[1] + ra[2] * t[2]), b2_ = xb[0] * t[0] + xb[1] * t[1] + xb[2] * t[2];
    const double det = a11 * a22 - a12 * a12;
    if (fabs(det) < 1e-18) return false;
    const double la = (b1_ * a22 - a12 * b2_) / det, lb = (a11 * b2_ - a12 * b1_) / det;
    return la > 0. && lb > 0. && la < 1e4 && lb < 1e4;
}

// ------------------------------------------------------------------------------------------------ host statements of the RANSAC loop
// The five indices of all max_samples samples, in the order estimateMotion draws them (five_point.hpp:568-586): the RNG is consumed by
// the picks only, so they do not depend on how many samples the stopping rule lets through.  n >= 5.
inline void draw_picks(uint64_t seed, int n, int max_samples, int32_t* picks /* [max_samples][5] */) {
    uint64_t state = seed * 0x9E3779B97F4A7C15ull + 0x1234567ull;
    for (int s = 0; s < max_samples; ++s) {
        int32_t* pick = picks + 5 * s;
        for (int q = 0; q < 5; ++q) {
            bool fresh;
            do {
                uint64_t x = (state += 0x9E3779B97F4A7C15ull);  // splitmix64
                x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
                x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
                x = x ^ (x >> 31);
                pick[q] = (int32_t)(x % (uint64_t)n);
                fresh = true;
                for (int r = 0; r < q; ++r) fresh = fresh && pick[r] != pick[q];
            } while (!fresh);
        }
    }
}

// pixel -> normalised image coordinates (:564-565)
inline double normalise(double p, double pp, double focal) { return (p - pp) / focal; }

// The stopping rule (:577, :595-611) over FULL inlier counts, applied after the fact: feed the samples in order, chunk by chunk.
// The host's early-abandoned count only shortens counts that cannot win, so the decisions are the same.
struct Scan {
    int need = 0, inliers = 0, samples = 0, best_sample = -1, best_model = -1;
    bool ok = false, done = false;
};
inline void scan_begin(Scan& sc, int max_samples) {
    sc = Scan();
    sc.need = max_samples;
}
// samples s0 .. s0 + len - 1: n_models[j] models of sample s0 + j with inlier counts counts[10 j + k].  Sets done when the loop of
// estimateMotion would have ended; samples of the chunk beyond that are ignored.
inline void scan_chunk(Scan& sc, int n, double probability, int max_samples, int s0, int len, const int32_t* n_models, const int32_t* counts) {
    for (int j = 0; j < len && !sc.done; ++j) {
        const int s = s0 + j;
        if (!(s < sc.need && s < max_samples)) {
            sc.done = true;
            break;
        }
        ++sc.samples;
        for (int k = 0; k < n_models[j]; ++k) {
            const int count = counts[10 * j + k];
            if (count > sc.inliers) {
                sc.inliers = count;
                sc.best_sample = s;
                sc.best_model = k;
                sc.ok = true;
                // samples needed for `probability` of one all-inlier sample at this inlier ratio (cv::RANSACUpdateNumIters)
                const double p5 = pow((double)count / (double)n, 5.);
                const double wr = p5 < 1. - 1e-12 ? p5 : 1. - 1e-12;
                const double num = 1. - probability, den = 1. - wr;
                const double k_ = log(1e-300 < num ? num : 1e-300) / log(1e-300 < den ? den : 1e-300);
                const double c = ceil(k_);
                const double lo = 1. < c ? c : 1.;
                sc.need = (int)(lo < (double)max_samples ? lo : (double)max_samples);
            }
        }
    }
    const int s = s0 + len;
    if (!(s < sc.need && s < max_samples)) sc.done = true;
}

}  // namespace fp5
}  // namespace kba
