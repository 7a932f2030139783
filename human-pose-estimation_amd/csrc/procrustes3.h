// procrustes3.h -- the 3x3 orthogonal Procrustes problem in double, for host and device (DESIGN.md "3-D pose scores"): the proper rotation
// R that maximises trace(R K) for K = sum_i x1_i x2_i^T, which is R = V diag(1, 1, sign det(U V^T)) U^T of K = U diag(s) V^T.
// Solved in Horn's quaternion form (B. K. P. Horn, "Closed-form solution of absolute orientation using unit quaternions", JOSA A 4, 1987):
// for a unit quaternion q of R, trace(R K) = q^T N q with the symmetric 4x4 matrix N below, so the optimum is N's largest eigenvalue and q
// an eigenvector of it.  Every unit quaternion is a proper rotation, so no reflection can come out and no determinant is ever tested; a
// rank-deficient K makes the largest eigenvalue multiple, and every eigenvector of it is optimal.  N's eigenvalues are the four sign
// combinations s1 +- s2 +- s3 with the product of the signs fixed, so the gap under the largest is 2 (s2 + s3 sign det): q, and R with it,
// is as well determined as that gap is wide.
// The eigenvectors come from cyclic Jacobi rotations: kSweeps sweeps over the six off-diagonal pairs, a fixed count (a symmetric 4x4
// matrix is diagonal to the last bit after 6 or 7), so the function terminates on any input.  K is scaled by its largest magnitude first,
// so 1e+150 does not overflow a square and 1e-150 does not vanish; a K that holds a NaN or an infinity gives NaN for R and the trace.
#pragma once

#ifndef __host__
#define __host__
#define __device__
#endif

namespace procrustes3 {

constexpr int kSweeps = 12;

// K, R row-major [9].  *trace_RK = sum_ij R[i][j] K[j][i], taken from the R that is returned.
__host__ __device__ inline void solve(const double K[9], double R[9], double* trace_RK) {
#pragma clang fp contract(off)
    double big = 0.0;
    bool finite = true;
    for (int i = 0; i < 9; ++i) {
        const double a = K[i] < 0.0 ? -K[i] : K[i];
        if (!(a <= 1.7976931348623157e308)) finite = false;  // NaN and infinity both fail the comparison
        if (a > big) big = a;
    }
    if (!finite) {
        const double nan = __builtin_nan("");
        for (int i = 0; i < 9; ++i) R[i] = nan;
        *trace_RK = nan;
        return;
    }
    const double div = big > 0.0 ? big : 1.0;  // a division: the reciprocal of a subnormal is infinite
    const double Sxx = K[0] / div, Sxy = K[1] / div, Sxz = K[2] / div, Syx = K[3] / div, Syy = K[4] / div, Syz = K[5] / div, Szx = K[6] / div,
                 Szy = K[7] / div, Szz = K[8] / div;
    double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
#pragma unroll 1
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                // tan of the rotation angle: the smaller root of t^2 + 2 theta t - 1 = 0; theta may overflow to infinity, t is then 0
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double at = theta < 0.0 ? -theta : theta;
                double t = 1.0 / (at + __builtin_sqrt(at * at + 1.0));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / __builtin_sqrt(t * t + 1.0), s = t * c;
                A[p][p] -= t * apq;
                A[q][q] += t * apq;
                A[p][q] = A[q][p] = 0.0;
                for (int r = 0; r < 4; ++r) {
                    if (r != p && r != q) {
                        const double arp = A[r][p], arq = A[r][q];
                        A[r][p] = A[p][r] = c * arp - s * arq;
                        A[r][q] = A[q][r] = s * arp + c * arq;
                    }
                    const double vrp = V[r][p], vrq = V[r][q];
                    V[r][p] = c * vrp - s * vrq;
                    V[r][q] = s * vrp + c * vrq;
                }
            }
        }
    }
    // the eigenvector of the largest eigenvalue (the first of equals), picked by selects: no array is indexed by a run-time value
    double top = A[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (A[i][i] > top) top = A[i][i], w = V[0][i], x = V[1][i], y = V[2][i], z = V[3][i];
    const double n = 1.0 / __builtin_sqrt(w * w + x * x + y * y + z * z);
    w *= n, x *= n, y *= n, z *= n;
    R[0] = w * w + x * x - y * y - z * z;
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);
    R[4] = w * w - x * x + y * y - z * z;
    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);
    R[7] = 2.0 * (y * z + w * x);
    R[8] = w * w - x * x - y * y + z * z;
    double tr = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) tr += R[3 * i + j] * K[3 * j + i];
    *trace_RK = tr;
}

}  // namespace procrustes3
