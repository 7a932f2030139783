// procrustes_host_check.cpp -- the 3x3 Procrustes solver of csrc/procrustes3.h on the host alone, under the sanitizers:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o procrustes_host_check tools/procrustes_host_check.cpp
//     ./procrustes_host_check
//
// Random, rank-deficient, mirrored, huge, tiny and NaN matrices.  For every finite K: R^T R = I and det R = +1 to 1e-12, and trace(R K) is
// not below that of 1000 random rotations (less 1e-12 |K|_F) nor of the identity.  For a K with a NaN or an infinity: NaN everywhere.
// No device, no library of the project, nothing of Python.  Exit status 0 and "procrustes_host_check OK" when every check holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../human-pose-estimation_amd/csrc/procrustes3.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
double uniform() {  // xorshift64*, in (0, 1)
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return ((rng_state * 0x2545F4914F6CDD1Dull >> 11) + 0.5) / 9007199254740992.0;
}
double normal() { return std::sqrt(-2.0 * std::log(uniform())) * std::cos(6.283185307179586 * uniform()); }

void random_rotation(double R[9]) {  // a uniformly random unit quaternion
    double q[4], n = 0;
    for (double& v : q) v = normal(), n += v * v;
    n = 1.0 / std::sqrt(n);
    const double w = q[0] * n, x = q[1] * n, y = q[2] * n, z = q[3] * n;
    const double M[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                         2 * (y * z - w * x),     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    for (int i = 0; i < 9; ++i) R[i] = M[i];
}

double trace_RK(const double R[9], const double K[9]) {
    double t = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) t += R[3 * i + j] * K[3 * j + i];
    return t;
}

int failures = 0;
long checked = 0;

void fail(const char* what, const char* family, const double K[9], double got) {
    if (++failures <= 10) {
        std::fprintf(stderr, "FAIL %s (%s): %.17g  K =", what, family, got);
        for (int i = 0; i < 9; ++i) std::fprintf(stderr, " %.17g", K[i]);
        std::fprintf(stderr, "\n");
    }
}

void check(const double K[9], const char* family) {
    double R[9], tr;
    procrustes3::solve(K, R, &tr);
    ++checked;
    bool finite = true;
    double frob = 0;
    for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(K[i]), frob += K[i] * K[i];
    if (!finite) {
        for (int i = 0; i < 9; ++i)
            if (!std::isnan(R[i])) fail("R is not NaN for a non-finite K", family, K, R[i]);
        if (!std::isnan(tr)) fail("trace is not NaN for a non-finite K", family, K, tr);
        return;
    }
    frob = std::sqrt(frob);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double d = 0;
            for (int k = 0; k < 3; ++k) d += R[3 * k + i] * R[3 * k + j];
            if (!(std::fabs(d - (i == j)) <= 1e-12)) fail("R^T R != I", family, K, d);
        }
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    if (!(std::fabs(det - 1.0) <= 1e-12)) fail("det R != +1", family, K, det);
    if (!(std::fabs(tr - trace_RK(R, K)) <= 1e-12 * frob)) fail("the returned trace is not trace(R K)", family, K, tr);
    const double slack = 1e-12 * frob;
    if (!(tr >= K[0] + K[4] + K[8] - slack)) fail("trace(R K) below the identity's", family, K, tr);
    for (int n = 0; n < 1000; ++n) {
        double Q[9];
        random_rotation(Q);
        const double tq = trace_RK(Q, K);
        if (!(tr >= tq - slack)) {
            fail("trace(R K) below a random rotation's", family, K, tr - tq);
            break;
        }
    }
}

void outer(const double a[3], const double b[3], double s, double K[9]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) K[3 * i + j] += s * a[i] * b[j];
}

}  // namespace

int main() {
    double K[9];
    for (int n = 0; n < 2000; ++n) {
        for (double& v : K) v = normal();
        check(K, "random");
        double M[9];  // mirrored: the optimal orthogonal matrix of D Q is a reflection
        random_rotation(M);
        const double s[3] = {1.0 + uniform(), 0.5 + 0.5 * uniform(), -(0.1 + 0.4 * uniform())};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) K[3 * i + j] = s[i] * M[3 * i + j];
        check(K, "mirrored");
        double a[3], b[3], c[3], d[3];
        for (int i = 0; i < 3; ++i) a[i] = normal(), b[i] = normal(), c[i] = normal(), d[i] = normal();
        for (double& v : K) v = 0;
        outer(a, b, 1.0, K);
        check(K, "rank 1");
        outer(c, d, uniform(), K);
        check(K, "rank 2");
        const double scales[] = {1e-300, 1e-150, 1e-12, 1e12, 1e150, 1e300};
        for (double sc : scales) {
            double S[9];
            for (int i = 0; i < 9; ++i) S[i] = K[i] * sc;
            check(S, "scaled rank 2");
            for (double& v : S) v = normal() * sc;
            check(S, "scaled random");
        }
        for (double& v : K) v = normal();
        K[n % 9] = (n & 1) ? NAN : (n & 2) ? INFINITY : -INFINITY;
        check(K, "non-finite");
    }
    for (double& v : K) v = 0;
    check(K, "zero");
    const double diag[][3] = {{1, 1, 1}, {1, 1, -1}, {-1, -1, -1}, {1, 0, 0}, {-1, 0, 0}, {0, 0, -1}, {1, 1, 0}, {2, 1, -1}, {1, 1, -1e-300}, {5e-324, 0, 0}};
    for (const auto& dg : diag) {
        for (double& v : K) v = 0;
        K[0] = dg[0], K[4] = dg[1], K[8] = dg[2];
        check(K, "diagonal");
    }
    if (failures) {
        std::fprintf(stderr, "procrustes_host_check: %d failure(s) in %ld matrices\n", failures, checked);
        return 1;
    }
    std::printf("procrustes_host_check OK: %ld matrices\n", checked);
    return 0;
}
